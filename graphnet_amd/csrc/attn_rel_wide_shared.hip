// graphnet_amd/csrc/attn_rel_wide_shared.hip — the two-lane spacetime-bias attention of attn_rel_wide.hip (head width 64) with
// each pair's sinusoidal embedding s_ij evaluated ONCE for a group of G heads, as attn_rel_shared.hip does at head width 32.
// s_ij depends on the two pulses only; attn_rel_wide.hip forms it per (tile, head): 16 sine / cosine pairs per lane and
// pair of pulses in each of the three passes.  Same mathematics, same pair-argument contract (attn_rel.hpp), same plan
// (gn_attention_plan), the same bits as attn_rel_wide.hip; another work split.
//
// Work split.  One workgroup of 2 G waves per (64-row tile of the plan, group of G heads), grid (tiles, ceil(H / G)).  The
// wave pair (2 g, 2 g + 1) serves head head0 + g as the two waves of an attn_rel_wide.hip workgroup do: the wave of parity w
// owns rows 32 w .. 32 w + 31 of the tile, lanes l and l ^ 32 are the halves h = l / 32 of one row; half h holds the row-side
// columns [32 h, 32 h + 32) and the frequencies [16 h, 16 h + 16); partial dot products meet through v_permlane32_swap as
// half0 + half1.  A (row, half) pair is a "unit": unit = 64 w + lane, 128 per tile, the same in every wave pair.
//
// Per block of G rows of the other side of the event:  (1) wave pair g PRODUCES block row g: every lane evaluates, for
// its own unit, what attn_rel_wide.hip evaluates for itself (rel_pair_arg on the same operands, the hi / lo frequency table of
// its half, 16 rel_sincos) and writes the 32 values to LDS; the pulse columns of that row are wave-uniform and are fetched one
// block ahead.  All threads together stage the block's K / V rows (forward, dQ) or q, q', dO, dU, lse2, delta rows (dK / dV)
// of the G heads.  (2) barrier.  (3) every wave CONSUMES all rows of the block for its head: it reads its own unit's s_ij
// back and goes on as attn_rel_wide.hip does once it has sc[]: bias terms first (ascending k, sine then cosine), the row-side
// terms in ascending column, the exchange between the halves, the online softmax key by key, delta summed as dA.
// (4) barrier before the next block overwrites the buffers.
//
// LDS.  s_ij of a block row is [chunk j < 8][unit < 128][4 floats] (16 KB); chunk j holds values 4 j .. 4 j + 3 of the unit
// (sines of its 16 frequencies, then the cosines), so the producer's ds_write_b128 and the consumers' ds_read_b128 touch
// consecutive 16 bytes on consecutive lanes.  The staged rows are [row][head of the group][64] and are read as broadcasts,
// two addresses per wave (one per half).  So is the frequency table (hi + lo of f_k / 2 pi, formed in double as in
// attn_rel_wide.hip, [half][16 hi | 16 lo], 256 B): in registers its 32 values per lane cost the dQ pass 72 and the dK / dV
// pass 32 bytes of scratch.  G = 4, single-buffered:
//   forward, dQ pass:  4 x 16 KB of s_ij + K and V 2 x 4 KB + table                          =  73,984 bytes
//   dK / dV pass:      4 x 16 KB of s_ij + q, q', dO, dU 4 x 4 KB + lse2, delta 128 B + table =  82,304 bytes
// of the 160 KB of a compute unit.  One workgroup per CU: its 8 waves, two per SIMD, have 256 registers each, which the
// dQ pass needs (six 32-wide row vectors are 192; the compiled kernel has 249).
//
// Barriers.  The trip count nb of the block loop depends on the event alone (kbeg, kend).  Both barriers of an iteration are
// outside every condition on the head, the row, the lane or the half.  A wave pair whose head is >= H (H = 1, H = 3, the last
// group of H = 9) still produces its block row and meets every barrier; it skips consuming and storing.  Lanes past the
// end of a short tile compute on the event's last row and store nothing.  The one `return` (a tile past the plan's last)
// depends on blockIdx.x alone: the workgroup leaves as a whole before its first barrier.
//
// fp32 operands and accumulation, no atomics, no matrix instructions (the per-head summation order is what makes the
// results those of attn_rel_wide.hip bit for bit), no packed fp32 operations.
#include "attn_rel.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int WS_DH = 64;                          // head width
constexpr int WS_HALF = 32;                        // floats of every vector per lane
constexpr int WS_HF = 16;                          // frequencies per lane
constexpr int WS_UNITS = 2 * REL_TILE;             // (row, half) units of a tile
constexpr int WS_SROW = WS_HALF * WS_UNITS;        // floats of s_ij per block row: [8 chunks][128 units][4]
constexpr int WS_G = 4;                            // heads per workgroup (wave pairs), all three kernels

// hi + lo of f_k / 2 pi (the double arithmetic of rel_freq_table) -> LDS [half][16 hi | 16 lo], by threads 0 .. 31.  The first
// barrier of the block loop stands between this and the first ws_produce.
__device__ __forceinline__ void ws_freq_table(float* __restrict__ Fs, const float* __restrict__ freq, int tid) {
    if (tid < 2 * WS_HF) {
        const double g = (double)freq[tid] * 0.15915494309189534561;
        const float hi = (float)g;
        float* f = Fs + (tid / WS_HF) * 2 * WS_HF + tid % WS_HF;
        f[0] = hi;
        f[WS_HF] = (float)(g - (double)hi);
    }
}

// s_ij of this unit = [16 sines | 16 cosines] of pair argument a -> its 8 chunks of the block row at srow; ft is the
// frequency table of the unit's half (two broadcast addresses per wave)
__device__ __forceinline__ void ws_produce(float* __restrict__ srow, float a, const float* __restrict__ ft, int unit) {
#pragma unroll
    for (int j = 0; j < WS_HF / 4; ++j) {                      // four frequencies: sine chunk j, cosine chunk 4 + j; 8 values live
        const float4 hi = *reinterpret_cast<const float4*>(ft + 4 * j);
        const float4 lo = *reinterpret_cast<const float4*>(ft + WS_HF + 4 * j);
        float sn[4], cs[4];
        rel_sincos(a, hi.x, lo.x, sn[0], cs[0]);
        rel_sincos(a, hi.y, lo.y, sn[1], cs[1]);
        rel_sincos(a, hi.z, lo.z, sn[2], cs[2]);
        rel_sincos(a, hi.w, lo.w, sn[3], cs[3]);
        *reinterpret_cast<float4*>(srow + (j * WS_UNITS + unit) * 4) = make_float4(sn[0], sn[1], sn[2], sn[3]);
        *reinterpret_cast<float4*>(srow + ((WS_HF / 4 + j) * WS_UNITS + unit) * 4) = make_float4(cs[0], cs[1], cs[2], cs[3]);
    }
}

// rows [r0, r0 + G) (clamped to r_last) of the G heads from head0 (clamped to H - 1: a column past the last head would leave
// the row) at column col0 + head * 64 -> LDS [row][head of the group][64]: G G 16 float4, one per thread t < G G 16.  With
// 128 G threads and G < 8 a tensor does not need them all; the callers rotate t so that the tensors spread over the waves.
template <int G>
__device__ __forceinline__ void ws_stage(float* __restrict__ dst, const float* __restrict__ src, long long ld, int col0, int head0,
                                         int H, int r0, int r_last, int t) {
    static_assert(G * G * 16 <= 128 * G, "one float4 per thread");
    if (t < G * G * 16) {
        const int r = t / (G * 16), j = (t / 16) % G, c4 = t % 16;
        const int row = min(r0 + r, r_last), hh = min(head0 + j, H - 1);
        *reinterpret_cast<float4*>(dst + t * 4) = *reinterpret_cast<const float4*>(src + (long long)row * ld + col0 + hh * WS_DH + c4 * 4);
    }
}

// Tile -> event and rows (the plan of gn_attention_plan), wave -> (head of the group, parity), lane -> (row, half).  `hc` is
// the head whose rows an idle wave pair loads; `tswap` is the thread index rotated by half a workgroup (ws_stage).
#define WS_PROLOGUE(ROW0, ROWI)                                                                                 \
    constexpr int NT = 128 * G;                                                                                 \
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;                                            \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                  \
    REL_EVENT_PROLOGUE(ROW0)                                                                                    \
    const int E = H * WS_DH;                                                                                    \
    const int g = wave >> 1, half = lane >> 5;                                                                  \
    const int unit = (wave & 1) * 64 + lane;                                                                    \
    const int ROWI = ROW0 + (wave & 1) * 32 + (lane & 31);                                                      \
    const bool valid = ROWI < kend;                                                                             \
    const int myrow = valid ? ROWI : kend - 1;                                                                  \
    const int head0 = blockIdx.y * G, head = head0 + g;                                                         \
    const bool active = head < H;                             /* wave-uniform */                                \
    const int hc = active ? head : H - 1;                                                                       \
    const int crow = hc * WS_DH + WS_HALF * half;             /* first row-side column of this lane */          \
    const int cemb = hc * WS_DH + WS_HF * half;               /* first sine column; the cosines start 32 further */ \
    (void)cemb;                                               /* the dK / dV pass has no embedding row of its own */ \
    const int tswap = tid < NT / 2 ? tid + NT / 2 : tid - NT / 2;                                               \
    const int nb = (kend - kbeg + G - 1) / G;                 /* blocks of the event: the same for every thread */

template <int G>
__global__ __launch_bounds__(128 * G) void rel_attn_wide_shared_fwd_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, float* __restrict__ out, long long ldo,
    float* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    extern __shared__ __attribute__((aligned(16))) float ws_lds[];
    float* const Ss = ws_lds;                                 // [G rows][8][128][4]
    float* const Ks = Ss + G * WS_SROW;                       // [G rows][G heads][64]
    float* const Vs = Ks + G * G * WS_DH;
    float* const Fs = Vs + G * G * WS_DH;                     // [2 halves][16 hi | 16 lo]
    WS_PROLOGUE(q0, qi)
    ws_freq_table(Fs, freq, tid);
    const float* const ft = Fs + half * 2 * WS_HF;
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    float q[WS_HALF], qq[WS_HALF], o[WS_HALF], uu[WS_HALF];
    rel_load_row(q, qkv + (long long)myrow * ld + crow, scale2);
    rel_load_emb(qq, qp + (long long)myrow * ldqp + cemb, REL_LOG2E);
#pragma unroll
    for (int d = 0; d < WS_HALF; ++d) { o[d] = 0.0f; uu[d] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + g, kend - 1));              // the row this wave pair produces, one block ahead
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * G;
        __syncthreads();                                      // every wave is done with the previous block
        ws_stage<G>(Ks, qkv, ld, E, head0, H, kb, kend - 1, tid);
        ws_stage<G>(Vs, qkv, ld, 2 * E, head0, H, kb, kend - 1, tswap);
        if (kb + g < kend) ws_produce(Ss + g * WS_SROW, rel_pair_arg(xi, xk), ft, unit);
        xk = rel_load_xt(xt, ldxt, min(kb + G + g, kend - 1));
        __syncthreads();                                      // the block is complete
        if (active) {
            const int nk = min(G, kend - kb);
            for (int c = 0; c < nk; ++c) {
                float sc[WS_HALF];
                rel_read<WS_HALF, WS_UNITS>(sc, Ss + c * WS_SROW, unit);
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < WS_HF; ++k) {
                    acc = fmaf(qq[k], sc[k], acc);
                    acc = fmaf(qq[WS_HF + k], sc[WS_HF + k], acc);
                }
                const float* kr = Ks + (c * G + g) * WS_DH + WS_HALF * half;
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    acc = fmaf(q[4 * d4], kk.x, acc); acc = fmaf(q[4 * d4 + 1], kk.y, acc);
                    acc = fmaf(q[4 * d4 + 2], kk.z, acc); acc = fmaf(q[4 * d4 + 3], kk.w, acc);
                }
                acc = rel_pair_sum(acc);                         // the score, the same bits on both halves
                if (acc > m) {                                  // a new maximum: rescale what has been summed so far
                    const float corr = exp2f(m - acc);
                    l *= corr;
#pragma unroll
                    for (int d = 0; d < WS_HALF; ++d) { o[d] *= corr; uu[d] *= corr; }
                    m = acc;
                }
                const float p = exp2f(acc - m);
                l += p;
                const float* vr = Vs + (c * G + g) * WS_DH + WS_HALF * half;
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                    o[4 * d4] = fmaf(p, vv.x, o[4 * d4]); o[4 * d4 + 1] = fmaf(p, vv.y, o[4 * d4 + 1]);
                    o[4 * d4 + 2] = fmaf(p, vv.z, o[4 * d4 + 2]); o[4 * d4 + 3] = fmaf(p, vv.w, o[4 * d4 + 3]);
                }
#pragma unroll
                for (int d = 0; d < WS_HALF; ++d) uu[d] = fmaf(p, sc[d], uu[d]);
            }
        }
    }
    if (valid && active) {
        const float inv = 1.0f / l;
        rel_store_row(out + (long long)qi * ldo + crow, o, inv);
        rel_store_emb(u + (long long)qi * ldu + cemb, uu, inv);
        if (half == 0) lse2[(long long)qi * H + head] = m + log2f(l);
    }
}

// dQ / dQ' pass: two lanes = one query.  Also writes delta[i, h] = dO_i . O_i + dU_i . U_i for the dK / dV pass.  Six row
// halves are 192 of the 256 registers a wave has at two waves per SIMD, so s_ij is not held across
// a key: it is read from LDS for the score / dA and again for dq', and a scheduling fence after every 16-byte chunk keeps
// the compiler from hoisting a key's LDS reads ahead of its multiply-adds (as in attn_rel_shared.hip).
template <int G>
__global__ __launch_bounds__(128 * G) void rel_attn_wide_shared_bwd_dq_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ out, long long ldo,
    const float* __restrict__ u, long long ldu, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq, float* __restrict__ dqp, long long lddqp) {
    extern __shared__ __attribute__((aligned(16))) float ws_lds[];
    float* const Ss = ws_lds;
    float* const Ks = Ss + G * WS_SROW;
    float* const Vs = Ks + G * G * WS_DH;
    float* const Fs = Vs + G * G * WS_DH;                     // [2 halves][16 hi | 16 lo]
    WS_PROLOGUE(q0, qi)
    ws_freq_table(Fs, freq, tid);
    const float* const ft = Fs + half * 2 * WS_HF;
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float q[WS_HALF], qq[WS_HALF], go[WS_HALF], gu[WS_HALF], dq[WS_HALF], dqq[WS_HALF];
    rel_load_row(q, qkv + (long long)myrow * ld + crow, scale2);
    rel_load_emb(qq, qp + (long long)myrow * ldqp + cemb, REL_LOG2E);
    rel_load_row(go, dout + (long long)myrow * lddo + crow, 1.0f);
    rel_load_emb(gu, du + (long long)myrow * lddu + cemb, 1.0f);
    float dl = 0.0f;
    {
        // delta = dU . U + dO . O, per half in the order in which dA = dU . s + dO . v is summed per key below, then the same
        // half0 + half1: with a single key (U = s, O = v bit for bit) dA - delta is exactly 0
        float t[WS_HALF];
        rel_load_emb(t, u + (long long)myrow * ldu + cemb, 1.0f);
#pragma unroll
        for (int k = 0; k < WS_HF; ++k) { dl = fmaf(gu[k], t[k], dl); dl = fmaf(gu[WS_HF + k], t[WS_HF + k], dl); }
        rel_load_row(t, out + (long long)myrow * ldo + crow, 1.0f);
#pragma unroll
        for (int d = 0; d < WS_HALF; ++d) dl = fmaf(go[d], t[d], dl);
        dl = rel_pair_sum(dl);
    }
#pragma unroll
    for (int d = 0; d < WS_HALF; ++d) { dq[d] = 0.0f; dqq[d] = 0.0f; }
    const float ls = lse2[(long long)myrow * H + hc];
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + g, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * G;
        __syncthreads();
        ws_stage<G>(Ks, qkv, ld, E, head0, H, kb, kend - 1, tid);
        ws_stage<G>(Vs, qkv, ld, 2 * E, head0, H, kb, kend - 1, tswap);
        if (kb + g < kend) ws_produce(Ss + g * WS_SROW, rel_pair_arg(xi, xk), ft, unit);
        xk = rel_load_xt(xt, ldxt, min(kb + G + g, kend - 1));
        __syncthreads();
        if (active) {
            const int nk = min(G, kend - kb);
            for (int c = 0; c < nk; ++c) {
                const float* sr = Ss + c * WS_SROW + unit * 4;
                float s = 0.0f, dp = 0.0f;
#pragma unroll
                for (int j = 0; j < WS_HF / 4; ++j) {          // four frequencies at a time: their sines, then their cosines
                    const float4 sn = *reinterpret_cast<const float4*>(sr + j * WS_UNITS * 4);
                    const float4 cs = *reinterpret_cast<const float4*>(sr + (WS_HF / 4 + j) * WS_UNITS * 4);
                    const int k = 4 * j;
                    s = fmaf(qq[k], sn.x, s); s = fmaf(qq[WS_HF + k], cs.x, s);
                    dp = fmaf(gu[k], sn.x, dp); dp = fmaf(gu[WS_HF + k], cs.x, dp);
                    s = fmaf(qq[k + 1], sn.y, s); s = fmaf(qq[WS_HF + k + 1], cs.y, s);
                    dp = fmaf(gu[k + 1], sn.y, dp); dp = fmaf(gu[WS_HF + k + 1], cs.y, dp);
                    s = fmaf(qq[k + 2], sn.z, s); s = fmaf(qq[WS_HF + k + 2], cs.z, s);
                    dp = fmaf(gu[k + 2], sn.z, dp); dp = fmaf(gu[WS_HF + k + 2], cs.z, dp);
                    s = fmaf(qq[k + 3], sn.w, s); s = fmaf(qq[WS_HF + k + 3], cs.w, s);
                    dp = fmaf(gu[k + 3], sn.w, dp); dp = fmaf(gu[WS_HF + k + 3], cs.w, dp);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const float* kr = Ks + (c * G + g) * WS_DH + WS_HALF * half;
                const float* vr = Vs + (c * G + g) * WS_DH + WS_HALF * half;
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                    s = fmaf(q[4 * d4], kk.x, s); s = fmaf(q[4 * d4 + 1], kk.y, s);
                    s = fmaf(q[4 * d4 + 2], kk.z, s); s = fmaf(q[4 * d4 + 3], kk.w, s);
                    dp = fmaf(go[4 * d4], vv.x, dp); dp = fmaf(go[4 * d4 + 1], vv.y, dp);
                    dp = fmaf(go[4 * d4 + 2], vv.z, dp); dp = fmaf(go[4 * d4 + 3], vv.w, dp);
                    __builtin_amdgcn_sched_barrier(0);
                }
                s = rel_pair_sum(s);
                dp = rel_pair_sum(dp);
                const float dS = exp2f(s - ls) * (dp - dl);
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    dq[4 * d4] = fmaf(dS, kk.x, dq[4 * d4]); dq[4 * d4 + 1] = fmaf(dS, kk.y, dq[4 * d4 + 1]);
                    dq[4 * d4 + 2] = fmaf(dS, kk.z, dq[4 * d4 + 2]); dq[4 * d4 + 3] = fmaf(dS, kk.w, dq[4 * d4 + 3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int j = 0; j < WS_HALF / 4; ++j) {
                    const float4 sv = *reinterpret_cast<const float4*>(sr + j * WS_UNITS * 4);
                    dqq[4 * j] = fmaf(dS, sv.x, dqq[4 * j]); dqq[4 * j + 1] = fmaf(dS, sv.y, dqq[4 * j + 1]);
                    dqq[4 * j + 2] = fmaf(dS, sv.z, dqq[4 * j + 2]); dqq[4 * j + 3] = fmaf(dS, sv.w, dqq[4 * j + 3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    if (valid && active) {
        rel_store_row(dqkv + (long long)qi * lddq + crow, dq, scale);
        rel_store_emb(dqp + (long long)qi * lddqp + cemb, dqq, 1.0f);
        if (half == 0) delta[(long long)qi * H + head] = dl;
    }
}

// dK / dV pass: two lanes = one key; the event's queries (q, q', dO, dU, lse2, delta of the G heads, and s_ij) pass through LDS
// G rows at a time - attn_rel_wide.hip streams 32 for one head; the per-lane summation order (queries ascending) does not
// depend on it.
template <int G>
__global__ __launch_bounds__(128 * G) void rel_attn_wide_shared_bwd_dkv_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq) {
    extern __shared__ __attribute__((aligned(16))) float ws_lds[];
    float* const Ss = ws_lds;                                 // [G rows][8][128][4]
    float* const Qs = Ss + G * WS_SROW;                       // [G rows][G heads][64] each
    float* const Ps = Qs + G * G * WS_DH;
    float* const Gs = Ps + G * G * WS_DH;
    float* const Us = Gs + G * G * WS_DH;
    float* const Ls = Us + G * G * WS_DH;                     // [G rows][G heads] each
    float* const Ds = Ls + G * G;
    float* const Fs = Ds + G * G;                             // [2 halves][16 hi | 16 lo]
    WS_PROLOGUE(k0, kj)
    ws_freq_table(Fs, freq, tid);
    const float* const ft = Fs + half * 2 * WS_HF;
    const float4 xj = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float k[WS_HALF], v[WS_HALF], dk[WS_HALF], dv[WS_HALF];
    rel_load_row(k, qkv + (long long)myrow * ld + E + crow, scale2);
    rel_load_row(v, qkv + (long long)myrow * ld + 2 * E + crow, 1.0f);
#pragma unroll
    for (int d = 0; d < WS_HALF; ++d) { dk[d] = 0.0f; dv[d] = 0.0f; }
    float4 xq = rel_load_xt(xt, ldxt, min(kbeg + g, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int qb = kbeg + b * G;
        __syncthreads();
        ws_stage<G>(Qs, qkv, ld, 0, head0, H, qb, kend - 1, tid);
        ws_stage<G>(Ps, qp, ldqp, 0, head0, H, qb, kend - 1, tswap);
        ws_stage<G>(Gs, dout, lddo, 0, head0, H, qb, kend - 1, tswap);
        ws_stage<G>(Us, du, lddu, 0, head0, H, qb, kend - 1, tid);
        if (tid < G * G) {
            const long long at = (long long)min(qb + tid / G, kend - 1) * H + min(head0 + tid % G, H - 1);
            Ls[tid] = lse2[at];
            Ds[tid] = delta[at];
        }
        if (qb + g < kend) ws_produce(Ss + g * WS_SROW, rel_pair_arg(xq, xj), ft, unit);           // query - key
        xq = rel_load_xt(xt, ldxt, min(qb + G + g, kend - 1));
        __syncthreads();
        if (active) {
            const int nq = min(G, kend - qb);
            for (int c = 0; c < nq; ++c) {
                float sc[WS_HALF];
                rel_read<WS_HALF, WS_UNITS>(sc, Ss + c * WS_SROW, unit);
                const float* qr = Qs + (c * G + g) * WS_DH + WS_HALF * half;
                const float* gr = Gs + (c * G + g) * WS_DH + WS_HALF * half;
                const float* pr = Ps + (c * G + g) * WS_DH + WS_HF * half;         // sines; the cosines 32 further
                const float* ur = Us + (c * G + g) * WS_DH + WS_HF * half;
                float bias = 0.0f, dp = 0.0f;
#pragma unroll
                for (int kk = 0; kk < WS_HF; ++kk) {
                    bias = fmaf(pr[kk], sc[kk], bias); bias = fmaf(pr[32 + kk], sc[WS_HF + kk], bias);
                    dp = fmaf(ur[kk], sc[kk], dp); dp = fmaf(ur[32 + kk], sc[WS_HF + kk], dp);
                }
                float s = bias * REL_LOG2E;
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                    const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                    s = fmaf(k[4 * d4], qv.x, s); s = fmaf(k[4 * d4 + 1], qv.y, s);
                    s = fmaf(k[4 * d4 + 2], qv.z, s); s = fmaf(k[4 * d4 + 3], qv.w, s);
                    dp = fmaf(v[4 * d4], gg.x, dp); dp = fmaf(v[4 * d4 + 1], gg.y, dp);
                    dp = fmaf(v[4 * d4 + 2], gg.z, dp); dp = fmaf(v[4 * d4 + 3], gg.w, dp);
                }
                s = rel_pair_sum(s);
                dp = rel_pair_sum(dp);
                const float p = exp2f(s - Ls[c * G + g]);
                const float dS = p * (dp - Ds[c * G + g]);
#pragma unroll
                for (int d4 = 0; d4 < WS_HALF / 4; ++d4) {
                    const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                    const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                    dv[4 * d4] = fmaf(p, gg.x, dv[4 * d4]); dv[4 * d4 + 1] = fmaf(p, gg.y, dv[4 * d4 + 1]);
                    dv[4 * d4 + 2] = fmaf(p, gg.z, dv[4 * d4 + 2]); dv[4 * d4 + 3] = fmaf(p, gg.w, dv[4 * d4 + 3]);
                    dk[4 * d4] = fmaf(dS, qv.x, dk[4 * d4]); dk[4 * d4 + 1] = fmaf(dS, qv.y, dk[4 * d4 + 1]);
                    dk[4 * d4 + 2] = fmaf(dS, qv.z, dk[4 * d4 + 2]); dk[4 * d4 + 3] = fmaf(dS, qv.w, dk[4 * d4 + 3]);
                }
            }
        }
    }
    if (valid && active) {
        rel_store_row(dqkv + (long long)kj * lddq + E + crow, dk, scale);
        rel_store_row(dqkv + (long long)kj * lddq + 2 * E + crow, dv, 1.0f);
    }
}
#undef WS_PROLOGUE

bool rel_attn_wide_shared_supported(int DH) { return DH == WS_DH; }

// s_ij, K, V (forward, dQ) or s_ij, q, q', dO, dU, lse2, delta (dK / dV), and the frequency table
constexpr int WS_LDS_QK = (WS_G * (WS_SROW + 2 * WS_G * WS_DH) + 4 * WS_HF) * 4;
constexpr int WS_LDS_KV = (WS_G * (WS_SROW + 4 * WS_G * WS_DH + 2 * WS_G) + 4 * WS_HF) * 4;
static_assert(WS_LDS_QK == 73984 && WS_LDS_KV == 82304, "the figures of the file header");
static_assert(WS_LDS_KV <= 160 * 1024, "one workgroup's LDS");

hipError_t launch_rel_attn_wide_shared_fwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                           long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr,
                                           int B, int N, void* out, long long ldo, void* u, long long ldu, float* lse2,
                                           hipStream_t st) {
    if (!rel_attn_wide_shared_supported(DH) || !rel_args_ok(false, 4, H, DH, ld, ldqp, ldxt, ldo, ldu)) return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once = rel_allow_lds(&rel_attn_wide_shared_fwd_kernel<WS_G>, WS_LDS_QK);
    if (once != hipSuccess) return once;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)((H + WS_G - 1) / WS_G)), block(128 * WS_G);
    hipLaunchKernelGGL((rel_attn_wide_shared_fwd_kernel<WS_G>), grid, block, WS_LDS_QK, st, (const float*)qkv, ld, (const float*)qp,
                       ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, rel_scale2(DH), (float*)out, ldo, (float*)u, ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_wide_shared_bwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                           long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr,
                                           int B, int N, const void* out, long long ldo, const void* u, long long ldu,
                                           const void* dout, long long lddo, const void* du, long long lddu, const float* lse2,
                                           float* delta, void* dqkv, long long lddq, void* dqp, long long lddqp, hipStream_t st) {
    if (!rel_attn_wide_shared_supported(DH) || !rel_args_ok(true, 4, H, DH, ld, ldqp, ldxt, ldo, ldu, lddo, lddu, lddq, lddqp))
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once_dq = rel_allow_lds(&rel_attn_wide_shared_bwd_dq_kernel<WS_G>, WS_LDS_QK);
    static const hipError_t once_kv = rel_allow_lds(&rel_attn_wide_shared_bwd_dkv_kernel<WS_G>, WS_LDS_KV);
    if (once_dq != hipSuccess) return once_dq;
    if (once_kv != hipSuccess) return once_kv;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)((H + WS_G - 1) / WS_G)), block(128 * WS_G);
    const float scale = rel_scale(DH);
    hipLaunchKernelGGL((rel_attn_wide_shared_bwd_dq_kernel<WS_G>), grid, block, WS_LDS_QK, st, (const float*)qkv, ld,
                       (const float*)qp, ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, scale, (const float*)out, ldo, (const float*)u,
                       ldu, (const float*)dout, lddo, (const float*)du, lddu, lse2, delta, (float*)dqkv, lddq, (float*)dqp, lddqp);
    hipLaunchKernelGGL((rel_attn_wide_shared_bwd_dkv_kernel<WS_G>), grid, block, WS_LDS_KV, st, (const float*)qkv, ld,
                       (const float*)qp, ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, scale, (const float*)dout, lddo,
                       (const float*)du, lddu, lse2, delta, (float*)dqkv, lddq);
    return hipGetLastError();
}

}  // namespace gn
