// graphnet_amd/csrc/attn_rel_mfma_wide.hip — the spacetime-bias attention at head width 64 with bf16 operands on the matrix
// cores: the fifth kernel family.  Same mathematics, same pair-argument contract (attn_rel.hpp), same plan (gn_attention_plan);
// s_ij (32 sines | 32 cosines) is formed in fp32 exactly as attn_rel_wide.hip forms it and rounded ONCE to bf16, P and dS are
// rounded to bf16 before their products, softmax statistics, delta and all accumulation are fp32.  DESIGN.md section 7t.
//
// Work split.  The layout of attn_rel_mfma.hip (32 owned rows) needs 208 KB of LDS at this width, so a workgroup owns HALF as
// many rows: one workgroup of 8 waves per (QUARTER of a 64-row tile of the plan = 16 rows, group of G = 16 heads), grid
// (4 tiles, ceil(H / 16)).  The other side of the event is walked in blocks of 16 rows, so a block is 16 x 16 = 256 pairs and
// TWO threads form each pair's s_ij: waves 0 .. 3 the frequencies 0 .. 15, waves 4 .. 7 the frequencies 16 .. 31 (the half is
// wave-uniform, so the frequency table stays in scalar registers).  Two kinds of product with two accumulator layouts:
//   per HEAD  (wave w: heads 2 w, 2 w + 1 of the group; TWO v_mfma_f32_16x16x32_bf16 over the head width per 16x16 score tile,
//       FOUR v_mfma_f32_16x16x16_bf16 over a block, one per 16-wide column tile of the head)
//       S^T[key][query] = K Q^T,  O^T[d][query] += V^T P^T,  dP^T = V dO^T,  dq^T += K^T dS^T  (dK / dV pass: S = Q K^T, dP = dO V^T,
//       dv^T[d][key] += dO^T P,  dk^T += Q^T dS).  The accumulator of a 16x16 product holds column l & 15 and rows 4 (l >> 4) + r,
//       which is the B-operand layout of the 16x16x16 product that follows: P and dS never leave their lanes on this side.
//   per QUERY (wave w: queries 2 w, 2 w + 1 of the 16; M = the 16 heads of the group, of which H = 12 leaves four rows idle)
//       bias[head][key] = q'_i s_i^T,  dAb = dU_i s_i^T  (2 x 16x16x32),   U_i[head][c] += P_i s_i,  dq'_i += dS_i s_i  (4 x 16x16x16).
// The two sides index (head, query, key) differently, so per block the bias scores (fp32, x log2 e), the bias part of dA
// (fp32), P or dS (bf16) and the online-softmax rescale factors (fp32) change layout through LDS.  Transposed operands
// (V^T, K^T, s_i as [key][c] -> B[k = key][c]) come out of row-major LDS tiles through ds_read_b64_tr_b16.
//
// Per block (forward; the dQ pass is the same with two exchanges, the dK / dV pass has no fourth step):
//   barrier A | all threads: K, V rows of the block (prefetched a block ahead in registers) -> LDS, thread t forms 16 sines and
//   16 cosines of pair (query (t & 255) / 16, key t % 16) -> LDS as bf16 | barrier B | per query: bias -> X | barrier C |
//   per head: scores, online softmax, O^T; P -> LDS, rescale factors -> LDS | barrier D | per query: U_i = U_i corr + P_i s_i.
//
// Barriers.  The trip count of the block loop depends on the event alone; every barrier stands outside any condition on the
// head, the row or the lane.  Heads past H - 1 compute on head H - 1 and rows past the event on its last row (every load is
// clamped), and store nothing.  The two `return`s depend on blockIdx.x and the event alone: a workgroup leaves as a whole
// before its first barrier.  No atomics; no packed fp32 operations.
#include "attn_rel_mfma.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int RX_DH = 64;                          // head width
constexpr int RX_HF = 16;                          // frequencies a thread forms: half of the 32
constexpr int RX_G = 16;                           // heads per workgroup = M of the per-query products
constexpr int RX_ROWS = 16;                        // rows a workgroup owns: a quarter of a tile of the plan
constexpr int RX_KB = 16;                          // rows of the other side per block
constexpr int RX_NT = 512;                         // threads: two per pair of a block
constexpr int RX_NC = RX_DH / 16;                  // 16-wide column tiles of a head
constexpr int RX_PC = RX_KB * RX_G * RX_DH / 8 / RX_NT;   // 16-byte pieces of a staged block per thread

// the two k halves (columns 32 kh + 8 (l >> 4) .. + 7) of a 64-wide row as the operands of two 16x16x32 products
__device__ __forceinline__ void rx_ld64(bf16x8 (&r)[2], const __bf16* p, int g4) {
    r[0] = rm_ld8(p + 8 * g4);
    r[1] = rm_ld8(p + 32 + 8 * g4);
}
// a[16 x 64] b[16 x 64]^T: the 16x16 tile over the whole head width
__device__ __forceinline__ f32x4 rx_dot64(const bf16x8 (&a)[2], const bf16x8 (&b)[2]) {
    f32x4 c;
    rm_zero(c);
    c = rm_mma32(a[0], b[0], c);
    return rm_mma32(a[1], b[1], c);
}

// this thread's half of s_ij = [32 sines | 32 cosines] of pair argument a, each value rounded once to bf16: sines to columns
// [16 fh, 16 fh + 16) and cosines to [32 + 16 fh, ..) of the pair's 64 columns at dst (2 x 32 bytes)
__device__ __forceinline__ void rx_produce(__bf16* __restrict__ dst, int fh, float a, const float (&ghi)[RX_HF], const float (&glo)[RX_HF]) {
#pragma unroll
    for (int j = 0; j < RX_HF / 8; ++j) {
        bf16x8 vs, vc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float sn, cs;
            rel_sincos(a, ghi[8 * j + i], glo[8 * j + i], sn, cs);
            vs[i] = (__bf16)sn; vc[i] = (__bf16)cs;
        }
        *reinterpret_cast<bf16x8*>(dst + RX_HF * fh + 8 * j) = vs;
        *reinterpret_cast<bf16x8*>(dst + RX_DH / 2 + RX_HF * fh + 8 * j) = vc;
    }
}

// rows [row0, row0 + 16) (clamped to r_last) of the 16 heads from head0 (clamped to H - 1) at column col0 + head * 64, by all
// 512 threads: four 16-byte pieces each, held in registers until rx_put writes them to LDS [row][head of the group][64]
__device__ __forceinline__ void rx_fetch(bf16x8 (&r)[RX_PC], const __bf16* __restrict__ src, long long ld, int col0, int head0, int H,
                                         int row0, int r_last, int tid) {
#pragma unroll
    for (int it = 0; it < RX_PC; ++it) {
        const int idx = it * RX_NT + tid;
        const int row = min(row0 + (idx >> 7), r_last), hh = min(head0 + ((idx >> 3) & 15), H - 1);
        r[it] = rm_ld8(src + (long long)row * ld + col0 + hh * RX_DH + (idx & 7) * 8);
    }
}
__device__ __forceinline__ void rx_put(__bf16* __restrict__ dst, const bf16x8 (&r)[RX_PC], int tid) {
#pragma unroll
    for (int it = 0; it < RX_PC; ++it) *reinterpret_cast<bf16x8*>(dst + (it * RX_NT + tid) * 8) = r[it];
}

// Quarter tile -> event and rows (the plan of gn_attention_plan).  li / g4: column and row group of a lane in a 16x16 product;
// fh: the half of the frequencies this wave forms; pa / pb: the pair of the block this thread forms (row / column of s_ij).
#define RX_PROLOGUE                                                                                             \
    const int tile = blockIdx.x >> 2, tid = threadIdx.x, lane = tid & 63;                                       \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                  \
    REL_EVENT_PROLOGUE(t0)                                                                                      \
    const int r0 = t0 + RX_ROWS * (int)(blockIdx.x & 3);                                                        \
    if (r0 >= kend) return;                                   /* this quarter of the tile lies past the event */ \
    const int E = H * RX_DH, li = lane & 15, g4 = lane >> 4;                                                    \
    const int head0 = blockIdx.y * RX_G;                                                                        \
    const int nb = (kend - kbeg + RX_KB - 1) / RX_KB;         /* blocks of the event: the same for every thread */ \
    const int fh = wave >> 2, pa = (tid >> 4) & 15, pb = tid & 15;                                              \
    float ghi[RX_HF], glo[RX_HF];                                                                               \
    rel_freq_table<RX_HF>(freq, fh, lane, ghi, glo);

// LDS, bytes.  forward: s_ij, X, P, K, V, corr;  dQ pass: s_ij, X, Y, dS, K, V;  dK / dV pass: s_ij, X, Y, Q, dO, lse2, delta
constexpr int RX_B_S = RX_ROWS * RX_KB * RX_DH * 2;        // 32 KB  s_ij of a block, bf16 [row][row of the other side][64]
constexpr int RX_B_X = RX_G * RX_ROWS * RX_KB * 4;         // 16 KB  fp32 exchange [head][..][..]
constexpr int RX_B_P = RX_ROWS * RX_G * RX_KB * 2;         //  8 KB  P / dS, bf16 [query][head][key]
constexpr int RX_B_R = RX_KB * RX_G * RX_DH * 2;           // 32 KB  staged rows, bf16 [row][head][64]
constexpr int RX_B_C = RX_ROWS * RX_G * 4;                 //  1 KB  per (query, head) factors
constexpr int RX_LDS_FWD = RX_B_S + RX_B_X + RX_B_P + 2 * RX_B_R + RX_B_C;                // 121 KB
constexpr int RX_LDS_DQ = RX_B_S + 2 * RX_B_X + RX_B_P + 2 * RX_B_R;                      // 136 KB
constexpr int RX_LDS_KV = RX_B_S + 2 * RX_B_X + 2 * RX_B_R + 2 * RX_KB * RX_G * 4;        // 130 KB
static_assert(RX_LDS_FWD <= 160 * 1024, "forward: one workgroup's LDS");
static_assert(RX_LDS_DQ <= 160 * 1024, "dQ pass: one workgroup's LDS");
static_assert(RX_LDS_KV <= 160 * 1024, "dK / dV pass: one workgroup's LDS");
static_assert(RX_PC * RX_NT * 8 == RX_KB * RX_G * RX_DH && RX_ROWS * RX_KB * 2 == RX_NT, "staging and pair split");

__global__ __launch_bounds__(RX_NT) void rel_attn_mfma_wide_fwd_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, __bf16* __restrict__ out, long long ldo,
    __bf16* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rx_lds);                               // [16 q][16 key][64]
    float* const Xs = reinterpret_cast<float*>(rx_lds + RX_B_S);                        // [16 head][16 q][16 key]
    __bf16* const Ps = reinterpret_cast<__bf16*>(rx_lds + RX_B_S + RX_B_X);             // [16 q][16 head][16 key]
    __bf16* const Ks = reinterpret_cast<__bf16*>(rx_lds + RX_B_S + RX_B_X + RX_B_P);    // [16 key][16 head][64]
    __bf16* const Vs = Ks + RX_B_R / 2;
    float* const Cs = reinterpret_cast<float*>(rx_lds + RX_B_S + RX_B_X + RX_B_P + 2 * RX_B_R);   // [16 q][16 head]
    RX_PROLOGUE
    const float4 xi = rel_load_xt(xt, ldxt, min(r0 + pa, kend - 1));
    // per query: q' of queries 2 w + t, row = head li of the group
    bf16x8 qpf[2][2];
    f32x4 uu[2][RX_NC];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        rx_ld64(qpf[t], qp + (long long)min(r0 + 2 * wave + t, kend - 1) * ldqp + min(head0 + li, H - 1) * RX_DH, g4);
#pragma unroll
        for (int n = 0; n < RX_NC; ++n) rm_zero(uu[t][n]);
    }
    // per head: q of heads 2 w + j, column = query li
    bf16x8 qf[2][2];
    f32x4 o[2][RX_NC];
    float m[2], l[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        rx_ld64(qf[j], qkv + (long long)min(r0 + li, kend - 1) * ld + min(head0 + 2 * wave + j, H - 1) * RX_DH, g4);
#pragma unroll
        for (int n = 0; n < RX_NC; ++n) rm_zero(o[j][n]);
        m[j] = -INFINITY; l[j] = 0.0f;
    }
    bf16x8 kn[RX_PC], vn[RX_PC];
    rx_fetch(kn, qkv, ld, E, head0, H, kbeg, kend - 1, tid);
    rx_fetch(vn, qkv, ld, 2 * E, head0, H, kbeg, kend - 1, tid);
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + pb, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * RX_KB;
        __syncthreads();                                      // A: every wave is done with the previous block
        rx_put(Ks, kn, tid);
        rx_put(Vs, vn, tid);
        rx_produce(Ss + (pa * RX_KB + pb) * RX_DH, fh, rel_pair_arg(xi, xk), ghi, glo);
        rx_fetch(kn, qkv, ld, E, head0, H, kb + RX_KB, kend - 1, tid);
        rx_fetch(vn, qkv, ld, 2 * E, head0, H, kb + RX_KB, kend - 1, tid);
        xk = rel_load_xt(xt, ldxt, min(kb + RX_KB + pb, kend - 1));
        __syncthreads();                                      // B: the block is complete
#pragma unroll
        for (int t = 0; t < 2; ++t) {                         // bias[head][key] of query 2 w + t, in the exp2 domain
            const int q = 2 * wave + t;
            bf16x8 sf[2];
            rx_ld64(sf, Ss + (q * RX_KB + li) * RX_DH, g4);
            const f32x4 d = rx_dot64(qpf[t], sf);
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[((4 * g4 + r) * RX_ROWS + q) * RX_KB + li] = d[r] * REL_LOG2E;
        }
        __syncthreads();                                      // C: the bias scores are in X
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j, q = li;
            bf16x8 kf[2];
            rx_ld64(kf, Ks + (li * RX_G + hl) * RX_DH, g4);
            const f32x4 s = rx_dot64(kf, qf[j]);              // S^T[key 4 g4 + r][query li]
            const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RX_ROWS + q) * RX_KB + 4 * g4);
            float sc[4] = {fmaf(s[0], scale2, x.x), fmaf(s[1], scale2, x.y), fmaf(s[2], scale2, x.z), fmaf(s[3], scale2, x.w)};
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kb + 4 * g4 + r >= kend) sc[r] = -INFINITY;
            float mx = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m[j], mx);                 // finite: key kb of every block exists
            const float corr = rm_exp2(m[j] - mn);
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = rm_exp2(sc[r] - mn);
            l[j] = fmaf(l[j], corr, (p[0] + p[1]) + (p[2] + p[3]));      // this lane's 4 keys; summed over g4 at the end
            m[j] = mn;
            const rm_s16x4 pv = rm_pack4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<rm_s16x4*>(Ps + (q * RX_G + hl) * RX_KB + 4 * g4) = pv;
            if (g4 == 0) Cs[q * RX_G + hl] = corr;
#pragma unroll
            for (int n = 0; n < RX_NC; ++n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) o[j][n][r] *= corr;
                o[j][n] = rm_mma16(rm_tr(Vs, RX_G * RX_DH, hl * RX_DH + 16 * n, lane), pv, o[j][n]);   // O^T[d 16 n + 4 g4 + r][query li]
            }
        }
        __syncthreads();                                      // D: P and the rescale factors are in LDS
#pragma unroll
        for (int t = 0; t < 2; ++t) {                         // U_i[head 4 g4 + r][c 16 n + li] of query 2 w + t
            const int q = 2 * wave + t;
            const float4 c = *reinterpret_cast<const float4*>(Cs + q * RX_G + 4 * g4);
            const rm_s16x4 pw = *reinterpret_cast<const rm_s16x4*>(Ps + (q * RX_G + li) * RX_KB + 4 * g4);
#pragma unroll
            for (int n = 0; n < RX_NC; ++n) {
                uu[t][n][0] *= c.x; uu[t][n][1] *= c.y; uu[t][n][2] *= c.z; uu[t][n][3] *= c.w;
                uu[t][n] = rm_mma16(pw, rm_tr(Ss + q * RX_KB * RX_DH, RX_DH, 16 * n, lane), uu[t][n]);
            }
        }
    }
    __syncthreads();                                          // the last block's factors have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int hl = 2 * wave + j, head = head0 + hl, q = li, qi = r0 + q;
        float lt = l[j];
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        const float inv = 1.0f / lt;
        if (g4 == 0) Cs[q * RX_G + hl] = inv;
        if (qi < kend && head < H) {
#pragma unroll
            for (int n = 0; n < RX_NC; ++n)
                rm_store4(out + (long long)qi * ldo + head * RX_DH + 16 * n + 4 * g4, o[j][n][0] * inv, o[j][n][1] * inv,
                          o[j][n][2] * inv, o[j][n][3] * inv);
            if (g4 == 0) lse2[(long long)qi * H + head] = m[j] + log2f(lt);
        }
    }
    __syncthreads();                                          // 1 / l of every (query, head) is in LDS
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int q = 2 * wave + t, qi = r0 + q;
        const float4 c = *reinterpret_cast<const float4*>(Cs + q * RX_G + 4 * g4);
        const float inv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int head = head0 + 4 * g4 + r;
            if (qi < kend && head < H) {
#pragma unroll
                for (int n = 0; n < RX_NC; ++n) u[(long long)qi * ldu + head * RX_DH + 16 * n + li] = (__bf16)(uu[t][n][r] * inv[r]);
            }
        }
    }
}

// dQ / dQ' pass: the workgroup owns 16 queries.  As the forward with two per-query products before the per-head step (bias and
// the bias part of dA) and dS in the place of P; scores are recomputed from lse2, nothing is rescaled.
__global__ __launch_bounds__(RX_NT) void rel_attn_mfma_wide_bwd_dq_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const __bf16* __restrict__ dout, long long lddo,
    const __bf16* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    __bf16* __restrict__ dqkv, long long lddq, __bf16* __restrict__ dqp, long long lddqp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rx_lds);                               // [16 q][16 key][64]
    float* const Xs = reinterpret_cast<float*>(rx_lds + RX_B_S);                        // [16 head][16 q][16 key]: bias log2 e
    float* const Ys = reinterpret_cast<float*>(rx_lds + RX_B_S + RX_B_X);               // the same: dU_i . s_ij
    __bf16* const Ps = reinterpret_cast<__bf16*>(rx_lds + RX_B_S + 2 * RX_B_X);         // [16 q][16 head][16 key]: dS
    __bf16* const Ks = reinterpret_cast<__bf16*>(rx_lds + RX_B_S + 2 * RX_B_X + RX_B_P);
    __bf16* const Vs = Ks + RX_B_R / 2;
    RX_PROLOGUE
    const float4 xi = rel_load_xt(xt, ldxt, min(r0 + pa, kend - 1));
    const float scale2 = scale * REL_LOG2E;
    bf16x8 qpf[2][2], duf[2][2];
    f32x4 dqq[2][RX_NC];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long long row = min(r0 + 2 * wave + t, kend - 1);
        const int col = min(head0 + li, H - 1) * RX_DH;
        rx_ld64(qpf[t], qp + row * ldqp + col, g4);
        rx_ld64(duf[t], du + row * lddu + col, g4);
#pragma unroll
        for (int n = 0; n < RX_NC; ++n) rm_zero(dqq[t][n]);
    }
    bf16x8 qf[2][2], gf[2][2];
    f32x4 dq[2][RX_NC];
    float ls[2], dl[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long row = min(r0 + li, kend - 1);
        const int hc = min(head0 + 2 * wave + j, H - 1);
        rx_ld64(qf[j], qkv + row * ld + hc * RX_DH, g4);
        rx_ld64(gf[j], dout + row * lddo + hc * RX_DH, g4);
        ls[j] = lse2[row * H + hc];
        dl[j] = delta[row * H + hc];
#pragma unroll
        for (int n = 0; n < RX_NC; ++n) rm_zero(dq[j][n]);
    }
    bf16x8 kn[RX_PC], vn[RX_PC];
    rx_fetch(kn, qkv, ld, E, head0, H, kbeg, kend - 1, tid);
    rx_fetch(vn, qkv, ld, 2 * E, head0, H, kbeg, kend - 1, tid);
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + pb, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * RX_KB;
        __syncthreads();                                      // A
        rx_put(Ks, kn, tid);
        rx_put(Vs, vn, tid);
        rx_produce(Ss + (pa * RX_KB + pb) * RX_DH, fh, rel_pair_arg(xi, xk), ghi, glo);
        __syncthreads();                                      // B
        rx_fetch(kn, qkv, ld, E, head0, H, kb + RX_KB, kend - 1, tid);      // the next block: in flight through steps B to D
        rx_fetch(vn, qkv, ld, 2 * E, head0, H, kb + RX_KB, kend - 1, tid);
        xk = rel_load_xt(xt, ldxt, min(kb + RX_KB + pb, kend - 1));
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q = 2 * wave + t;
            bf16x8 sf[2];
            rx_ld64(sf, Ss + (q * RX_KB + li) * RX_DH, g4);
            const f32x4 d = rx_dot64(qpf[t], sf), g = rx_dot64(duf[t], sf);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xs[((4 * g4 + r) * RX_ROWS + q) * RX_KB + li] = d[r] * REL_LOG2E;
                Ys[((4 * g4 + r) * RX_ROWS + q) * RX_KB + li] = g[r];
            }
        }
        __syncthreads();                                      // C
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j, q = li;
            bf16x8 kf[2], vf[2];
            rx_ld64(kf, Ks + (li * RX_G + hl) * RX_DH, g4);
            rx_ld64(vf, Vs + (li * RX_G + hl) * RX_DH, g4);
            const f32x4 s = rx_dot64(kf, qf[j]);              // S^T[key 4 g4 + r][query li]
            const f32x4 dp = rx_dot64(vf, gf[j]);             // (dO . v)^T
            const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RX_ROWS + q) * RX_KB + 4 * g4);
            const float4 y = *reinterpret_cast<const float4*>(Ys + (hl * RX_ROWS + q) * RX_KB + 4 * g4);
            const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
            float dS[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float p = rm_exp2(fmaf(s[r], scale2, xs[r]) - ls[j]);
                if (kb + 4 * g4 + r >= kend) p = 0.0f;
                dS[r] = p * ((dp[r] + ys[r]) - dl[j]);
            }
            const rm_s16x4 db = rm_pack4(dS[0], dS[1], dS[2], dS[3]);
            *reinterpret_cast<rm_s16x4*>(Ps + (q * RX_G + hl) * RX_KB + 4 * g4) = db;
#pragma unroll
            for (int n = 0; n < RX_NC; ++n)                   // dq^T[d 16 n + 4 g4 + r][query li]
                dq[j][n] = rm_mma16(rm_tr(Ks, RX_G * RX_DH, hl * RX_DH + 16 * n, lane), db, dq[j][n]);
        }
        __syncthreads();                                      // D
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q = 2 * wave + t;
            const rm_s16x4 pw = *reinterpret_cast<const rm_s16x4*>(Ps + (q * RX_G + li) * RX_KB + 4 * g4);
#pragma unroll
            for (int n = 0; n < RX_NC; ++n) dqq[t][n] = rm_mma16(pw, rm_tr(Ss + q * RX_KB * RX_DH, RX_DH, 16 * n, lane), dqq[t][n]);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int head = head0 + 2 * wave + j, qi = r0 + li;
        if (qi < kend && head < H) {
#pragma unroll
            for (int n = 0; n < RX_NC; ++n)
                rm_store4(dqkv + (long long)qi * lddq + head * RX_DH + 16 * n + 4 * g4, dq[j][n][0] * scale, dq[j][n][1] * scale,
                          dq[j][n][2] * scale, dq[j][n][3] * scale);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int qi = r0 + 2 * wave + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int head = head0 + 4 * g4 + r;
            if (qi < kend && head < H) {
#pragma unroll
                for (int n = 0; n < RX_NC; ++n) dqp[(long long)qi * lddqp + head * RX_DH + 16 * n + li] = (__bf16)dqq[t][n][r];
            }
        }
    }
}

// dK / dV pass: the workgroup owns 16 keys; the event's queries pass 16 at a time.  Per query (wave w: queries 2 w, 2 w + 1 of
// the block) bias and dU . s for the 16 keys; per head S = Q K^T and dP = dO V^T with the queries as rows, so that P and dS
// leave their accumulators as the B operands (k = query) of dv^T += dO^T P and dk^T += Q^T dS.  q' and dU of the block's
// queries are read where they are used, not a block ahead: the registers go to the 32 accumulator tiles of dk^T and dv^T.
__global__ __launch_bounds__(RX_NT) void rel_attn_mfma_wide_bwd_dkv_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const __bf16* __restrict__ dout, long long lddo,
    const __bf16* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    __bf16* __restrict__ dqkv, long long lddq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rx_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rx_lds);                               // [16 q][16 key][64]
    float* const Xs = reinterpret_cast<float*>(rx_lds + RX_B_S);                        // [16 head][16 key][16 q]: bias log2 e
    float* const Ys = reinterpret_cast<float*>(rx_lds + RX_B_S + RX_B_X);               // the same: dU_i . s_ij
    __bf16* const Qs = reinterpret_cast<__bf16*>(rx_lds + RX_B_S + 2 * RX_B_X);         // [16 q][16 head][64]
    __bf16* const Gs = Qs + RX_B_R / 2;                                                 // the same: dO
    float* const Ls = reinterpret_cast<float*>(rx_lds + RX_B_S + 2 * RX_B_X + 2 * RX_B_R);   // [16 q][16 head]
    float* const Ds = Ls + RX_KB * RX_G;
    RX_PROLOGUE                                                // pa: query of the block, pb: key
    const float4 xj = rel_load_xt(xt, ldxt, min(r0 + pb, kend - 1));
    const float scale2 = scale * REL_LOG2E;
    const int hq = min(head0 + li, H - 1) * RX_DH;             // per query: this lane's row of q' and dU
    // per head: k, v of heads 2 w + j, column = key li
    bf16x8 kf[2][2], vf[2][2];
    f32x4 dk[2][RX_NC], dv[2][RX_NC];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const long long row = min(r0 + li, kend - 1);
        const int hc = min(head0 + 2 * wave + j, H - 1);
        rx_ld64(kf[j], qkv + row * ld + E + hc * RX_DH, g4);
        rx_ld64(vf[j], qkv + row * ld + 2 * E + hc * RX_DH, g4);
#pragma unroll
        for (int n = 0; n < RX_NC; ++n) { rm_zero(dk[j][n]); rm_zero(dv[j][n]); }
    }
    // lse2 / delta of (query, head) = (pa, pb) of the block, by the first 256 threads (the others load the same again)
    const int sh = min(head0 + pb, H - 1);
    bf16x8 qn[RX_PC], gn_[RX_PC];
    rx_fetch(qn, qkv, ld, 0, head0, H, kbeg, kend - 1, tid);
    rx_fetch(gn_, dout, lddo, 0, head0, H, kbeg, kend - 1, tid);
    float ln = lse2[(long long)min(kbeg + pa, kend - 1) * H + sh];
    float dn = delta[(long long)min(kbeg + pa, kend - 1) * H + sh];
    float4 xq = rel_load_xt(xt, ldxt, min(kbeg + pa, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int qb = kbeg + b * RX_KB;
        __syncthreads();                                      // A
        rx_put(Qs, qn, tid);
        rx_put(Gs, gn_, tid);
        if (tid < RX_KB * RX_G) { Ls[tid] = ln; Ds[tid] = dn; }
        rx_produce(Ss + (pa * RX_ROWS + pb) * RX_DH, fh, rel_pair_arg(xq, xj), ghi, glo);      // query - key
        bf16x8 qpf[2][2], duf[2][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long row = min(qb + 2 * wave + t, kend - 1);
            rx_ld64(qpf[t], qp + row * ldqp + hq, g4);
            rx_ld64(duf[t], du + row * lddu + hq, g4);
        }
        rx_fetch(qn, qkv, ld, 0, head0, H, qb + RX_KB, kend - 1, tid);
        rx_fetch(gn_, dout, lddo, 0, head0, H, qb + RX_KB, kend - 1, tid);
        ln = lse2[(long long)min(qb + RX_KB + pa, kend - 1) * H + sh];
        dn = delta[(long long)min(qb + RX_KB + pa, kend - 1) * H + sh];
        xq = rel_load_xt(xt, ldxt, min(qb + RX_KB + pa, kend - 1));
        __syncthreads();                                      // B
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q = 2 * wave + t;
            bf16x8 sf[2];
            rx_ld64(sf, Ss + (q * RX_ROWS + li) * RX_DH, g4);
            const f32x4 d = rx_dot64(qpf[t], sf), g = rx_dot64(duf[t], sf);     // [head 4 g4 + r][key li]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xs[((4 * g4 + r) * RX_ROWS + li) * RX_KB + q] = d[r] * REL_LOG2E;
                Ys[((4 * g4 + r) * RX_ROWS + li) * RX_KB + q] = g[r];
            }
        }
        __syncthreads();                                      // C
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j;
            bf16x8 qa[2], ga[2];
            rx_ld64(qa, Qs + (li * RX_G + hl) * RX_DH, g4);
            rx_ld64(ga, Gs + (li * RX_G + hl) * RX_DH, g4);
            const f32x4 s = rx_dot64(qa, kf[j]);              // S[query 4 g4 + r][key li]
            const f32x4 dp = rx_dot64(ga, vf[j]);
            const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RX_ROWS + li) * RX_KB + 4 * g4);
            const float4 y = *reinterpret_cast<const float4*>(Ys + (hl * RX_ROWS + li) * RX_KB + 4 * g4);
            const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
            float p[4], dS[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = rm_exp2(fmaf(s[r], scale2, xs[r]) - Ls[(4 * g4 + r) * RX_G + hl]);
                if (qb + 4 * g4 + r >= kend) p[r] = 0.0f;
                dS[r] = p[r] * ((dp[r] + ys[r]) - Ds[(4 * g4 + r) * RX_G + hl]);
            }
            const rm_s16x4 pv = rm_pack4(p[0], p[1], p[2], p[3]), db = rm_pack4(dS[0], dS[1], dS[2], dS[3]);
#pragma unroll
            for (int n = 0; n < RX_NC; ++n) {                 // dv^T, dk^T[d 16 n + 4 g4 + r][key li]
                dv[j][n] = rm_mma16(rm_tr(Gs, RX_G * RX_DH, hl * RX_DH + 16 * n, lane), pv, dv[j][n]);
                dk[j][n] = rm_mma16(rm_tr(Qs, RX_G * RX_DH, hl * RX_DH + 16 * n, lane), db, dk[j][n]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int head = head0 + 2 * wave + j, kj = r0 + li;
        if (kj < kend && head < H) {
#pragma unroll
            for (int n = 0; n < RX_NC; ++n) {
                rm_store4(dqkv + (long long)kj * lddq + E + head * RX_DH + 16 * n + 4 * g4, dk[j][n][0] * scale, dk[j][n][1] * scale,
                          dk[j][n][2] * scale, dk[j][n][3] * scale);
                rm_store4(dqkv + (long long)kj * lddq + 2 * E + head * RX_DH + 16 * n + 4 * g4, dv[j][n][0], dv[j][n][1], dv[j][n][2],
                          dv[j][n][3]);
            }
        }
    }
}
#undef RX_PROLOGUE

bool rel_attn_mfma_wide_supported(int DH) { return DH == RX_DH; }

hipError_t launch_rel_attn_mfma_wide_fwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                         long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                         int N, void* out, long long ldo, void* u, long long ldu, float* lse2, hipStream_t st) {
    if (!rel_attn_mfma_wide_supported(DH) || !rel_args_ok(false, 8, H, DH, ld, ldqp, ldxt, ldo, ldu)) return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once = rel_allow_lds(&rel_attn_mfma_wide_fwd_kernel, RX_LDS_FWD);
    if (once != hipSuccess) return once;
    const dim3 grid((unsigned)(REL_TILE / RX_ROWS) * (unsigned)(N / REL_TILE + B), (unsigned)((H + RX_G - 1) / RX_G)), block(RX_NT);
    hipLaunchKernelGGL(rel_attn_mfma_wide_fwd_kernel, grid, block, RX_LDS_FWD, st, static_cast<const __bf16*>(qkv), ld,
                       static_cast<const __bf16*>(qp), ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, rel_scale2(DH),
                       static_cast<__bf16*>(out), ldo, static_cast<__bf16*>(u), ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_mfma_wide_bwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                         long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                         int N, const void* out, long long ldo, const void* u, long long ldu, const void* dout,
                                         long long lddo, const void* du, long long lddu, const float* lse2, float* delta, void* dqkv,
                                         long long lddq, void* dqp, long long lddqp, hipStream_t st) {
    if (!rel_attn_mfma_wide_supported(DH) || !rel_args_ok(true, 8, H, DH, ld, ldqp, ldxt, ldo, ldu, lddo, lddu, lddq, lddqp))
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once_dq = rel_allow_lds(&rel_attn_mfma_wide_bwd_dq_kernel, RX_LDS_DQ);
    static const hipError_t once_kv = rel_allow_lds(&rel_attn_mfma_wide_bwd_dkv_kernel, RX_LDS_KV);
    if (once_dq != hipSuccess) return once_dq;
    if (once_kv != hipSuccess) return once_kv;
    const __bf16* qkv_ = static_cast<const __bf16*>(qkv);
    const __bf16* qp_ = static_cast<const __bf16*>(qp);
    const __bf16* dout_ = static_cast<const __bf16*>(dout);
    const __bf16* du_ = static_cast<const __bf16*>(du);
    const long long NH = (long long)N * H;
    hipLaunchKernelGGL(rel_attn_mfma_delta_kernel<RX_DH>, dim3((unsigned)((NH + 255) / 256)), dim3(256), 0, st,
                       static_cast<const __bf16*>(out), ldo, static_cast<const __bf16*>(u), ldu, dout_, lddo, du_, lddu, H, NH, delta);
    const dim3 grid((unsigned)(REL_TILE / RX_ROWS) * (unsigned)(N / REL_TILE + B), (unsigned)((H + RX_G - 1) / RX_G)), block(RX_NT);
    const float scale = rel_scale(DH);
    hipLaunchKernelGGL(rel_attn_mfma_wide_bwd_dq_kernel, grid, block, RX_LDS_DQ, st, qkv_, ld, qp_, ldqp, xt, ldxt, freq, H, ptr,
                       tile_ptr, B, scale, dout_, lddo, du_, lddu, lse2, delta, static_cast<__bf16*>(dqkv), lddq,
                       static_cast<__bf16*>(dqp), lddqp);
    hipLaunchKernelGGL(rel_attn_mfma_wide_bwd_dkv_kernel, grid, block, RX_LDS_KV, st, qkv_, ld, qp_, ldqp, xt, ldxt, freq, H, ptr,
                       tile_ptr, B, scale, dout_, lddo, du_, lddu, lse2, delta, static_cast<__bf16*>(dqkv), lddq);
    return hipGetLastError();
}

}  // namespace gn
