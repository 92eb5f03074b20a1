// graphnet_amd/csrc/attn_rel_shared.hip — the spacetime-bias attention of attn_rel.hip (head width 32) with each pair's
// sinusoidal embedding s_ij evaluated ONCE for a group of W heads instead of once per head.  s_ij depends on the two pulses
// only; in attn_rel.hip every (tile, head) wave forms it for itself: 16 sine / cosine pairs of ~30 vector instructions
// against 128 multiply-adds of attention work, in each of the three passes.  Same mathematics, same pair-argument contract
// (attn_rel.hpp), same plan (gn_attention_plan), same results; another work split.
//
// Work split.  One workgroup of W waves per (64-row tile of the plan, group g of W heads), grid (tiles, ceil(H / W)).  Wave w
// serves head g W + w; lane l of every wave owns row l of the tile (a query in the forward and the dQ pass, a key in the
// dK / dV pass), as in attn_rel.hip.  The other side of the event is walked in blocks of KB = W rows.
//
// Per block:  (1) wave w PRODUCES the block's row w: every lane evaluates s_ij of its own row with that row - exactly
// the code of attn_rel.hip (rel_pair_arg, the hi / lo frequency table formed once per wave, rel_sincos) - and writes the 32
// values to LDS; all threads together stage the block's K / V rows (forward, dQ) or q, q', dO, dU, lse2, delta rows
// (dK / dV) of the W heads.  (2) barrier.  (3) every wave CONSUMES all rows of the block for its head: it reads its own
// lane's s_ij back and continues as the per-head kernel does after it has formed s_ij, in that kernel's order (online softmax
// key by key; bias terms first, ascending k, sine then cosine; then the row-side terms; delta summed as dA).  (4) barrier
// before the next block overwrites the buffers.
//
// LDS.  s_ij of a block row is [chunk j < 8][lane < 64][4 floats] (8 KB): chunk j holds columns 4 j .. 4 j + 3, so the
// producer's ds_write_b128 and the consumers' ds_read_b128 both touch consecutive 16 bytes on consecutive lanes - no bank
// conflict on either side.  The staged rows are [row][head of the group][32] and are read as broadcasts.  W = 8:
// forward / dQ 8 x (8 KB + 2 x 1 KB) = 80 KB, dK / dV 8 x (8 KB + 4 x 1 KB + 64 B) = 96.5 KB, one workgroup per CU (its 8 waves
// fill the register file at 256 registers each anyway).  A second s_ij buffer would need 2 x 64 KB + 2 x 16 KB = 160 KB, all
// there is, so the block is single-buffered with two barriers; the two waves a SIMD holds stand at different points of
// the block, which is what overlaps sines with multiply-adds.
//
// Barriers.  The trip count nb of the block loop depends on the event alone (kbeg, kend), which is the same for all threads
// of a workgroup; both barriers of an iteration are outside every condition on the head, the row or the lane.  A wave whose
// head is >= H (the last group of H = 9, five of the eight waves at H = 3) still produces its row and meets every barrier;
// it skips consuming and storing.  Lanes past the end of a short tile compute on the event's last row and store nothing.
// The one `return` (a tile past the plan's last) depends on blockIdx.x alone: a workgroup leaves as a whole before its first
// barrier.
//
// fp32 operands and accumulation, no atomics, no matrix instructions (a lane owns a whole row and the per-head summation
// order is what makes the results equal to attn_rel.hip's bit for bit), no packed fp32 operations.
#include "attn_rel.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int RS_DH = 32;                          // head width
constexpr int RS_HF = 16;                          // frequencies
constexpr int RS_SROW = RS_DH * REL_TILE;          // floats of s_ij per block row: [8 chunks][64 lanes][4]
constexpr int RS_W = 8;                            // heads per workgroup (waves), all three kernels

// s_ij = [sin | cos] of pair argument a -> this lane's 8 chunks of the block row at srow
__device__ __forceinline__ void rs_produce(float* __restrict__ srow, float a, const float (&ghi)[RS_HF], const float (&glo)[RS_HF],
                                           int lane) {
#pragma unroll
    for (int j = 0; j < RS_HF / 4; ++j) {                      // four frequencies: sine chunk j, cosine chunk 4 + j; 8 values live
        float sn[4], cs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rel_sincos(a, ghi[4 * j + i], glo[4 * j + i], sn[i], cs[i]);
        *reinterpret_cast<float4*>(srow + (j * REL_TILE + lane) * 4) = make_float4(sn[0], sn[1], sn[2], sn[3]);
        *reinterpret_cast<float4*>(srow + ((RS_HF / 4 + j) * REL_TILE + lane) * 4) = make_float4(cs[0], cs[1], cs[2], cs[3]);
    }
}

// rows [r0, r0 + W) (clamped to r_last) of the W heads from head0 (clamped to H - 1: a column past the last head would leave
// the row) at column col0 + head * 32 -> LDS [row][head of the group][32], by all 64 W threads
template <int W>
__device__ __forceinline__ void rs_stage(float* __restrict__ dst, const float* __restrict__ src, long long ld, int col0, int head0,
                                         int H, int r0, int r_last, int tid) {
    static_assert(W * W * 8 % (64 * W) == 0, "one float4 per thread and pass");
#pragma unroll
    for (int it = 0; it < W * W * 8 / (64 * W); ++it) {
        const int idx = it * 64 * W + tid;
        const int r = idx / (W * 8), j = (idx / 8) % W, c4 = idx % 8;
        const int row = min(r0 + r, r_last), hh = min(head0 + j, H - 1);
        *reinterpret_cast<float4*>(dst + idx * 4) = *reinterpret_cast<const float4*>(src + (long long)row * ld + col0 + hh * RS_DH + c4 * 4);
    }
}

// Tile -> event and rows (the plan of gn_attention_plan), wave -> head.  `hc` is the head whose rows an idle wave loads.
#define RS_PROLOGUE(ROW0, ROWI)                                                                                 \
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63;                                            \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                  \
    REL_EVENT_PROLOGUE(ROW0)                                                                                    \
    const int E = H * RS_DH;                                                                                    \
    const int ROWI = ROW0 + lane;                                                                               \
    const bool valid = ROWI < kend;                                                                             \
    const int myrow = valid ? ROWI : kend - 1;                                                                  \
    const int head0 = blockIdx.y * W, head = head0 + wave;                                                      \
    const bool active = head < H;                             /* wave-uniform */                                \
    const int hc = active ? head : H - 1;                                                                       \
    const int nb = (kend - kbeg + W - 1) / W;                 /* blocks of the event: the same for every thread */

template <int W>
__global__ __launch_bounds__(64 * W) void rel_attn_shared_fwd_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, float* __restrict__ out, long long ldo,
    float* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* const Ss = rs_lds;                                 // [W rows][8][64][4]
    float* const Ks = Ss + W * RS_SROW;                       // [W rows][W heads][32]
    float* const Vs = Ks + W * W * RS_DH;
    RS_PROLOGUE(q0, qi)
    float ghi[RS_HF], glo[RS_HF];
    rel_freq_table<RS_HF>(freq, 0, lane, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    float q[RS_DH], qq[RS_DH], o[RS_DH], uu[RS_DH];
    rel_load_row(q, qkv + (long long)myrow * ld + hc * RS_DH, scale2);
    rel_load_row(qq, qp + (long long)myrow * ldqp + hc * RS_DH, REL_LOG2E);
#pragma unroll
    for (int d = 0; d < RS_DH; ++d) { o[d] = 0.0f; uu[d] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + wave, kend - 1));           // the row this wave produces, one block ahead
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * W;
        __syncthreads();                                      // every wave is done with the previous block
        rs_stage<W>(Ks, qkv, ld, E, head0, H, kb, kend - 1, tid);
        rs_stage<W>(Vs, qkv, ld, 2 * E, head0, H, kb, kend - 1, tid);
        if (kb + wave < kend) rs_produce(Ss + wave * RS_SROW, rel_pair_arg(xi, xk), ghi, glo, lane);
        xk = rel_load_xt(xt, ldxt, min(kb + W + wave, kend - 1));
        __syncthreads();                                      // the block is complete
        if (active) {
            const int nk = min(W, kend - kb);
            for (int c = 0; c < nk; ++c) {
                float sc[RS_DH];
                rel_read<RS_DH, REL_TILE>(sc, Ss + c * RS_SROW, lane);
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < RS_HF; ++k) {
                    acc = fmaf(qq[k], sc[k], acc);
                    acc = fmaf(qq[RS_HF + k], sc[RS_HF + k], acc);
                }
                const float* kr = Ks + (c * W + wave) * RS_DH;
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    acc = fmaf(q[4 * d4], kk.x, acc); acc = fmaf(q[4 * d4 + 1], kk.y, acc);
                    acc = fmaf(q[4 * d4 + 2], kk.z, acc); acc = fmaf(q[4 * d4 + 3], kk.w, acc);
                }
                if (acc > m) {                              // a new maximum: rescale what has been summed so far
                    const float corr = exp2f(m - acc);
                    l *= corr;
#pragma unroll
                    for (int d = 0; d < RS_DH; ++d) { o[d] *= corr; uu[d] *= corr; }
                    m = acc;
                }
                const float p = exp2f(acc - m);
                l += p;
                const float* vr = Vs + (c * W + wave) * RS_DH;
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
                    const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                    o[4 * d4] = fmaf(p, vv.x, o[4 * d4]); o[4 * d4 + 1] = fmaf(p, vv.y, o[4 * d4 + 1]);
                    o[4 * d4 + 2] = fmaf(p, vv.z, o[4 * d4 + 2]); o[4 * d4 + 3] = fmaf(p, vv.w, o[4 * d4 + 3]);
                }
#pragma unroll
                for (int d = 0; d < RS_DH; ++d) uu[d] = fmaf(p, sc[d], uu[d]);
            }
        }
    }
    if (valid && active) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
            *reinterpret_cast<float4*>(out + (long long)qi * ldo + head * RS_DH + d4 * 4) =
                make_float4(o[4 * d4] * inv, o[4 * d4 + 1] * inv, o[4 * d4 + 2] * inv, o[4 * d4 + 3] * inv);
            *reinterpret_cast<float4*>(u + (long long)qi * ldu + head * RS_DH + d4 * 4) =
                make_float4(uu[4 * d4] * inv, uu[4 * d4 + 1] * inv, uu[4 * d4 + 2] * inv, uu[4 * d4 + 3] * inv);
        }
        lse2[(long long)qi * H + head] = m + log2f(l);
    }
}

// dQ / dQ' pass: lane = query.  Also writes delta[i, h] = dO_i . O_i + dU_i . U_i for the dK / dV pass.  Six row vectors are
// 192 of the 256 registers a wave has at two waves per SIMD, so s_ij is not held across a key: it is read from LDS for the
// score / dA and again for dq', and a scheduling fence after every 16-byte chunk keeps the compiler from hoisting a key's
// 24 LDS reads ahead of its multiply-adds (without the fences: 256 registers and 96 bytes of scratch).
template <int W>
__global__ __launch_bounds__(64 * W) void rel_attn_shared_bwd_dq_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ out, long long ldo,
    const float* __restrict__ u, long long ldu, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq, float* __restrict__ dqp, long long lddqp) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* const Ss = rs_lds;
    float* const Ks = Ss + W * RS_SROW;
    float* const Vs = Ks + W * W * RS_DH;
    RS_PROLOGUE(q0, qi)
    float ghi[RS_HF], glo[RS_HF];
    rel_freq_table<RS_HF>(freq, 0, lane, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float q[RS_DH], qq[RS_DH], go[RS_DH], gu[RS_DH], dq[RS_DH], dqq[RS_DH];
    rel_load_row(q, qkv + (long long)myrow * ld + hc * RS_DH, scale2);
    rel_load_row(qq, qp + (long long)myrow * ldqp + hc * RS_DH, REL_LOG2E);
    rel_load_row(go, dout + (long long)myrow * lddo + hc * RS_DH, 1.0f);
    rel_load_row(gu, du + (long long)myrow * lddu + hc * RS_DH, 1.0f);
    float dl = 0.0f;
    {
        // delta = dU . U + dO . O, summed in the order in which dA = dU . s + dO . v is summed per key below: with a single
        // key (U = s, O = v bit for bit) dA - delta is then exactly 0, as the softmax of one score has no gradient
        float t[RS_DH];
        rel_load_row(t, u + (long long)myrow * ldu + hc * RS_DH, 1.0f);
#pragma unroll
        for (int k = 0; k < RS_HF; ++k) { dl = fmaf(gu[k], t[k], dl); dl = fmaf(gu[RS_HF + k], t[RS_HF + k], dl); }
        rel_load_row(t, out + (long long)myrow * ldo + hc * RS_DH, 1.0f);
#pragma unroll
        for (int d = 0; d < RS_DH; ++d) dl = fmaf(go[d], t[d], dl);
    }
#pragma unroll
    for (int d = 0; d < RS_DH; ++d) { dq[d] = 0.0f; dqq[d] = 0.0f; }
    const float ls = lse2[(long long)myrow * H + hc];
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + wave, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * W;
        __syncthreads();
        rs_stage<W>(Ks, qkv, ld, E, head0, H, kb, kend - 1, tid);
        rs_stage<W>(Vs, qkv, ld, 2 * E, head0, H, kb, kend - 1, tid);
        if (kb + wave < kend) rs_produce(Ss + wave * RS_SROW, rel_pair_arg(xi, xk), ghi, glo, lane);
        xk = rel_load_xt(xt, ldxt, min(kb + W + wave, kend - 1));
        __syncthreads();
        if (active) {
            const int nk = min(W, kend - kb);
            for (int c = 0; c < nk; ++c) {
                const float* sr = Ss + c * RS_SROW + lane * 4;
                float s = 0.0f, dp = 0.0f;
#pragma unroll
                for (int j = 0; j < RS_HF / 4; ++j) {          // four frequencies at a time: their sines, then their cosines
                    const float4 sn = *reinterpret_cast<const float4*>(sr + j * REL_TILE * 4);
                    const float4 cs = *reinterpret_cast<const float4*>(sr + (RS_HF / 4 + j) * REL_TILE * 4);
                    const int k = 4 * j;
                    s = fmaf(qq[k], sn.x, s); s = fmaf(qq[RS_HF + k], cs.x, s);
                    dp = fmaf(gu[k], sn.x, dp); dp = fmaf(gu[RS_HF + k], cs.x, dp);
                    s = fmaf(qq[k + 1], sn.y, s); s = fmaf(qq[RS_HF + k + 1], cs.y, s);
                    dp = fmaf(gu[k + 1], sn.y, dp); dp = fmaf(gu[RS_HF + k + 1], cs.y, dp);
                    s = fmaf(qq[k + 2], sn.z, s); s = fmaf(qq[RS_HF + k + 2], cs.z, s);
                    dp = fmaf(gu[k + 2], sn.z, dp); dp = fmaf(gu[RS_HF + k + 2], cs.z, dp);
                    s = fmaf(qq[k + 3], sn.w, s); s = fmaf(qq[RS_HF + k + 3], cs.w, s);
                    dp = fmaf(gu[k + 3], sn.w, dp); dp = fmaf(gu[RS_HF + k + 3], cs.w, dp);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const float* kr = Ks + (c * W + wave) * RS_DH;
                const float* vr = Vs + (c * W + wave) * RS_DH;
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                    s = fmaf(q[4 * d4], kk.x, s); s = fmaf(q[4 * d4 + 1], kk.y, s);
                    s = fmaf(q[4 * d4 + 2], kk.z, s); s = fmaf(q[4 * d4 + 3], kk.w, s);
                    dp = fmaf(go[4 * d4], vv.x, dp); dp = fmaf(go[4 * d4 + 1], vv.y, dp);
                    dp = fmaf(go[4 * d4 + 2], vv.z, dp); dp = fmaf(go[4 * d4 + 3], vv.w, dp);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const float dS = exp2f(s - ls) * (dp - dl);
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
                    const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                    dq[4 * d4] = fmaf(dS, kk.x, dq[4 * d4]); dq[4 * d4 + 1] = fmaf(dS, kk.y, dq[4 * d4 + 1]);
                    dq[4 * d4 + 2] = fmaf(dS, kk.z, dq[4 * d4 + 2]); dq[4 * d4 + 3] = fmaf(dS, kk.w, dq[4 * d4 + 3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int j = 0; j < RS_DH / 4; ++j) {
                    const float4 sv = *reinterpret_cast<const float4*>(sr + j * REL_TILE * 4);
                    dqq[4 * j] = fmaf(dS, sv.x, dqq[4 * j]); dqq[4 * j + 1] = fmaf(dS, sv.y, dqq[4 * j + 1]);
                    dqq[4 * j + 2] = fmaf(dS, sv.z, dqq[4 * j + 2]); dqq[4 * j + 3] = fmaf(dS, sv.w, dqq[4 * j + 3]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    if (valid && active) {
#pragma unroll
        for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
            *reinterpret_cast<float4*>(dqkv + (long long)qi * lddq + head * RS_DH + d4 * 4) =
                make_float4(dq[4 * d4] * scale, dq[4 * d4 + 1] * scale, dq[4 * d4 + 2] * scale, dq[4 * d4 + 3] * scale);
            *reinterpret_cast<float4*>(dqp + (long long)qi * lddqp + head * RS_DH + d4 * 4) =
                make_float4(dqq[4 * d4], dqq[4 * d4 + 1], dqq[4 * d4 + 2], dqq[4 * d4 + 3]);
        }
        delta[(long long)qi * H + head] = dl;
    }
}

// dK / dV pass: lane = key; the event's queries (q, q', dO, dU, lse2, delta of the W heads, and s_ij) pass through LDS W rows at
// a time - attn_rel.hip streams 32 for one head; the per-lane summation order (queries ascending) does not depend on it.
template <int W>
__global__ __launch_bounds__(64 * W) void rel_attn_shared_bwd_dkv_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* const Ss = rs_lds;                                 // [W rows][8][64][4]
    float* const Qs = Ss + W * RS_SROW;                       // [W rows][W heads][32] each
    float* const Ps = Qs + W * W * RS_DH;
    float* const Gs = Ps + W * W * RS_DH;
    float* const Us = Gs + W * W * RS_DH;
    float* const Ls = Us + W * W * RS_DH;                     // [W rows][W heads] each
    float* const Ds = Ls + W * W;
    RS_PROLOGUE(k0, kj)
    float ghi[RS_HF], glo[RS_HF];
    rel_freq_table<RS_HF>(freq, 0, lane, ghi, glo);
    const float4 xj = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float k[RS_DH], v[RS_DH], dk[RS_DH], dv[RS_DH];
    rel_load_row(k, qkv + (long long)myrow * ld + E + hc * RS_DH, scale2);
    rel_load_row(v, qkv + (long long)myrow * ld + 2 * E + hc * RS_DH, 1.0f);
#pragma unroll
    for (int d = 0; d < RS_DH; ++d) { dk[d] = 0.0f; dv[d] = 0.0f; }
    float4 xq = rel_load_xt(xt, ldxt, min(kbeg + wave, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int qb = kbeg + b * W;
        __syncthreads();
        rs_stage<W>(Qs, qkv, ld, 0, head0, H, qb, kend - 1, tid);
        rs_stage<W>(Ps, qp, ldqp, 0, head0, H, qb, kend - 1, tid);
        rs_stage<W>(Gs, dout, lddo, 0, head0, H, qb, kend - 1, tid);
        rs_stage<W>(Us, du, lddu, 0, head0, H, qb, kend - 1, tid);
        if (tid < W * W) {
            const long long at = (long long)min(qb + tid / W, kend - 1) * H + min(head0 + tid % W, H - 1);
            Ls[tid] = lse2[at];
            Ds[tid] = delta[at];
        }
        if (qb + wave < kend) rs_produce(Ss + wave * RS_SROW, rel_pair_arg(xq, xj), ghi, glo, lane);      // query - key
        xq = rel_load_xt(xt, ldxt, min(qb + W + wave, kend - 1));
        __syncthreads();
        if (active) {
            const int nq = min(W, kend - qb);
            for (int c = 0; c < nq; ++c) {
                float sc[RS_DH];
                rel_read<RS_DH, REL_TILE>(sc, Ss + c * RS_SROW, lane);
                const float* qr = Qs + (c * W + wave) * RS_DH;
                const float* pr = Ps + (c * W + wave) * RS_DH;
                const float* gr = Gs + (c * W + wave) * RS_DH;
                const float* ur = Us + (c * W + wave) * RS_DH;
                float bias = 0.0f, dp = 0.0f;
#pragma unroll
                for (int kk = 0; kk < RS_HF; ++kk) {
                    bias = fmaf(pr[kk], sc[kk], bias); bias = fmaf(pr[RS_HF + kk], sc[RS_HF + kk], bias);
                    dp = fmaf(ur[kk], sc[kk], dp); dp = fmaf(ur[RS_HF + kk], sc[RS_HF + kk], dp);
                }
                float s = bias * REL_LOG2E;
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
                    const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                    const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                    s = fmaf(k[4 * d4], qv.x, s); s = fmaf(k[4 * d4 + 1], qv.y, s);
                    s = fmaf(k[4 * d4 + 2], qv.z, s); s = fmaf(k[4 * d4 + 3], qv.w, s);
                    dp = fmaf(v[4 * d4], gg.x, dp); dp = fmaf(v[4 * d4 + 1], gg.y, dp);
                    dp = fmaf(v[4 * d4 + 2], gg.z, dp); dp = fmaf(v[4 * d4 + 3], gg.w, dp);
                }
                const float p = exp2f(s - Ls[c * W + wave]);
                const float dS = p * (dp - Ds[c * W + wave]);
#pragma unroll
                for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
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
#pragma unroll
        for (int d4 = 0; d4 < RS_DH / 4; ++d4) {
            *reinterpret_cast<float4*>(dqkv + (long long)kj * lddq + E + head * RS_DH + d4 * 4) =
                make_float4(dk[4 * d4] * scale, dk[4 * d4 + 1] * scale, dk[4 * d4 + 2] * scale, dk[4 * d4 + 3] * scale);
            *reinterpret_cast<float4*>(dqkv + (long long)kj * lddq + 2 * E + head * RS_DH + d4 * 4) =
                make_float4(dv[4 * d4], dv[4 * d4 + 1], dv[4 * d4 + 2], dv[4 * d4 + 3]);
        }
    }
}
#undef RS_PROLOGUE

bool rel_attn_shared_supported(int DH) { return DH == RS_DH; }

constexpr int RS_LDS_QK = RS_W * (RS_SROW + 2 * RS_W * RS_DH) * 4;                       // forward, dQ: s_ij, K, V
constexpr int RS_LDS_KV = RS_W * (RS_SROW + 4 * RS_W * RS_DH + 2 * RS_W) * 4;            // dK / dV: s_ij, q, q', dO, dU, lse2, delta
static_assert(RS_LDS_KV <= 160 * 1024, "one workgroup's LDS");

hipError_t launch_rel_attn_shared_fwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                      long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                      int N, void* out, long long ldo, void* u, long long ldu, float* lse2, hipStream_t st) {
    if (!rel_attn_shared_supported(DH) || !rel_args_ok(false, 4, H, DH, ld, ldqp, ldxt, ldo, ldu)) return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once = rel_allow_lds(&rel_attn_shared_fwd_kernel<RS_W>, RS_LDS_QK);
    if (once != hipSuccess) return once;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)((H + RS_W - 1) / RS_W)), block(64 * RS_W);
    hipLaunchKernelGGL((rel_attn_shared_fwd_kernel<RS_W>), grid, block, RS_LDS_QK, st, (const float*)qkv, ld, (const float*)qp, ldqp,
                       xt, ldxt, freq, H, ptr, tile_ptr, B, rel_scale2(DH), (float*)out, ldo, (float*)u, ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_shared_bwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                      long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                      int N, const void* out, long long ldo, const void* u, long long ldu, const void* dout,
                                      long long lddo, const void* du, long long lddu, const float* lse2, float* delta,
                                      void* dqkv, long long lddq, void* dqp, long long lddqp, hipStream_t st) {
    if (!rel_attn_shared_supported(DH) || !rel_args_ok(true, 4, H, DH, ld, ldqp, ldxt, ldo, ldu, lddo, lddu, lddq, lddqp))
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once_dq = rel_allow_lds(&rel_attn_shared_bwd_dq_kernel<RS_W>, RS_LDS_QK);
    static const hipError_t once_kv = rel_allow_lds(&rel_attn_shared_bwd_dkv_kernel<RS_W>, RS_LDS_KV);
    if (once_dq != hipSuccess) return once_dq;
    if (once_kv != hipSuccess) return once_kv;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)((H + RS_W - 1) / RS_W)), block(64 * RS_W);
    const float scale = rel_scale(DH);
    hipLaunchKernelGGL((rel_attn_shared_bwd_dq_kernel<RS_W>), grid, block, RS_LDS_QK, st, (const float*)qkv, ld, (const float*)qp,
                       ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, scale, (const float*)out, ldo, (const float*)u, ldu,
                       (const float*)dout, lddo, (const float*)du, lddu, lse2, delta, (float*)dqkv, lddq, (float*)dqp, lddqp);
    hipLaunchKernelGGL((rel_attn_shared_bwd_dkv_kernel<RS_W>), grid, block, RS_LDS_KV, st, (const float*)qkv, ld, (const float*)qp,
                       ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, scale, (const float*)dout, lddo, (const float*)du, lddu, lse2,
                       delta, (float*)dqkv, lddq);
    return hipGetLastError();
}

}  // namespace gn
