// graphnet_amd/csrc/attn_rel_mfma.hip — the spacetime-bias attention of attn_rel.hip (head width 32) with bf16 operands on the
// matrix cores: the fourth kernel family.  Same mathematics, same pair-argument contract (attn_rel.hpp), same plan
// (gn_attention_plan); s_ij is formed in fp32 exactly as in the other families and rounded ONCE to bf16, P and dS are rounded
// to bf16 before their products, softmax statistics, delta and all accumulation are fp32.  DESIGN.md section 7s.
//
// Work split.  One workgroup of 8 waves per (HALF a 64-row tile of the plan = 32 rows, group of G = 16 heads), grid
// (2 tiles, ceil(H / 16)).  The other side of the event is walked in blocks of 16 rows, so a block is 32 x 16 = 512 pairs:
// one pair per thread when s_ij is formed.  Two kinds of product with two accumulator layouts:
//   per HEAD  (wave w: heads 2 w, 2 w + 1 of the group; v_mfma_f32_16x16x32_bf16 over the head width, 16x16x16 over a block)
//       S^T[key][query] = K Q^T,  O^T[d][query] += V^T P^T,  dP^T = V dO^T,  dq^T += K^T dS^T  (dK / dV pass: S = Q K^T, dP = dO V^T,
//       dv^T[d][key] += dO^T P,  dk^T += Q^T dS).  The accumulator of a 16x16 product holds column l & 15 and rows 4 (l >> 4) + r,
//       which is the B-operand layout of the 16x16x16 product that follows: P and dS never leave their lanes on this side.
//   per QUERY (wave w: queries 4 w .. 4 w + 3 of the 32; M = the 16 heads of the group)
//       bias[head][key] = q'_i s_i^T,  dAb = dU_i s_i^T  (16x16x32),   U_i[head][c] += P_i s_i,  dq'_i += dS_i s_i  (16x16x16).
// The two sides index (head, query, key) differently, so per block the bias scores (fp32, x log2 e), the bias part of dA
// (fp32), P or dS (bf16) and the online-softmax rescale factors (fp32) change layout through LDS.  Transposed operands
// (V^T, K^T, s_i as [key][c] -> B[k = key][c]) come out of row-major LDS tiles through ds_read_b64_tr_b16.
//
// Per block (forward; the dQ pass is the same with two exchanges, the dK / dV pass has no fourth step):
//   barrier A | all threads: K, V rows of the block (prefetched a block ahead in registers) -> LDS, thread t forms s_ij of
//   pair (query t / 16, key t % 16) -> LDS as bf16 | barrier B | per query: bias -> X | barrier C | per head: scores,
//   online softmax, O^T; P -> LDS, rescale factors -> LDS | barrier D | per query: U_i = U_i corr + P_i s_i.
//
// Barriers.  The trip count of the block loop depends on the event alone; every barrier stands outside any condition on the
// head, the row or the lane.  Heads past H - 1 compute on head H - 1 and rows past the event on its last row (every load is
// clamped), and store nothing.  The two `return`s depend on blockIdx.x and the event alone: a workgroup leaves as a whole
// before its first barrier.  No atomics; no packed fp32 operations.
#include "attn_rel_mfma.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int RM_DH = 32;                          // head width
constexpr int RM_HF = 16;                          // frequencies
constexpr int RM_G = 16;                           // heads per workgroup = M of the per-query products
constexpr int RM_ROWS = 32;                        // rows a workgroup owns: half a tile of the plan
constexpr int RM_KB = 16;                          // rows of the other side per block
constexpr int RM_NT = 512;                         // threads: one pair of a block each

// s_ij = [sin | cos] of pair argument a, each value rounded once to bf16 -> the pair's 32 columns at dst (64 bytes)
__device__ __forceinline__ void rm_produce(__bf16* __restrict__ dst, float a, const float (&ghi)[RM_HF], const float (&glo)[RM_HF]) {
#pragma unroll
    for (int j = 0; j < RM_HF / 8; ++j) {
        bf16x8 vs, vc;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float sn, cs;
            rel_sincos(a, ghi[8 * j + i], glo[8 * j + i], sn, cs);
            vs[i] = (__bf16)sn; vc[i] = (__bf16)cs;
        }
        *reinterpret_cast<bf16x8*>(dst + 8 * j) = vs;
        *reinterpret_cast<bf16x8*>(dst + RM_HF + 8 * j) = vc;
    }
}

// rows [row0, row0 + 16) (clamped to r_last) of the 16 heads from head0 (clamped to H - 1) at column col0 + head * 32, by all
// 512 threads: two 16-byte pieces each, held in registers until rm_put writes them to LDS [row][head of the group][32]
__device__ __forceinline__ void rm_fetch(bf16x8 (&r)[2], const __bf16* __restrict__ src, long long ld, int col0, int head0, int H,
                                         int row0, int r_last, int tid) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = it * RM_NT + tid;
        const int row = min(row0 + (idx >> 6), r_last), hh = min(head0 + ((idx >> 2) & 15), H - 1);
        r[it] = rm_ld8(src + (long long)row * ld + col0 + hh * RM_DH + (idx & 3) * 8);
    }
}
__device__ __forceinline__ void rm_put(__bf16* __restrict__ dst, const bf16x8 (&r)[2], int tid) {
#pragma unroll
    for (int it = 0; it < 2; ++it) *reinterpret_cast<bf16x8*>(dst + (it * RM_NT + tid) * 8) = r[it];
}

// Half tile -> event and rows (the plan of gn_attention_plan).  li / g4: column and row group of a lane in a 16x16 product.
#define RM_PROLOGUE                                                                                             \
    const int tile = blockIdx.x >> 1, tid = threadIdx.x, lane = tid & 63;                                       \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                  \
    REL_EVENT_PROLOGUE(t0)                                                                                      \
    const int r0 = t0 + RM_ROWS * (int)(blockIdx.x & 1);                                                        \
    if (r0 >= kend) return;                                   /* the tile's second half lies past the event */  \
    const int E = H * RM_DH, li = lane & 15, g4 = lane >> 4;                                                    \
    const int head0 = blockIdx.y * RM_G;                                                                        \
    const int nb = (kend - kbeg + RM_KB - 1) / RM_KB;         /* blocks of the event: the same for every thread */

// LDS, bytes.  forward: s_ij, X, P, K, V, corr;  dQ pass: s_ij, X, Y, dS, K, V;  dK / dV pass: s_ij, X, Y, Q, dO, lse2, delta
constexpr int RM_B_S = RM_ROWS * RM_KB * RM_DH * 2;        // 32 KB  s_ij of a block, bf16 [row][row of the other side][32]
constexpr int RM_B_X = RM_G * RM_ROWS * RM_KB * 4;         // 32 KB  fp32 exchange [head][..][..]
constexpr int RM_B_P = RM_ROWS * RM_G * RM_KB * 2;         // 16 KB  P / dS, bf16 [query][head][key]
constexpr int RM_B_R = RM_KB * RM_G * RM_DH * 2;           // 16 KB  staged rows, bf16 [row][head][32]
constexpr int RM_B_C = RM_ROWS * RM_G * 4;                 //  2 KB  per (query, head) factors
constexpr int RM_LDS_FWD = RM_B_S + RM_B_X + RM_B_P + 2 * RM_B_R + RM_B_C;
constexpr int RM_LDS_DQ = RM_B_S + 2 * RM_B_X + RM_B_P + 2 * RM_B_R;
constexpr int RM_LDS_KV = RM_B_S + 2 * RM_B_X + 2 * RM_B_R + 2 * RM_KB * RM_G * 4;
static_assert(RM_LDS_FWD <= 160 * 1024 && RM_LDS_DQ <= 160 * 1024 && RM_LDS_KV <= 160 * 1024, "one workgroup's LDS");

__global__ __launch_bounds__(RM_NT) void rel_attn_mfma_fwd_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, __bf16* __restrict__ out, long long ldo,
    __bf16* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rm_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rm_lds);                               // [32 q][16 key][32]
    float* const Xs = reinterpret_cast<float*>(rm_lds + RM_B_S);                        // [16 head][32 q][16 key]
    __bf16* const Ps = reinterpret_cast<__bf16*>(rm_lds + RM_B_S + RM_B_X);             // [32 q][16 head][16 key]
    __bf16* const Ks = reinterpret_cast<__bf16*>(rm_lds + RM_B_S + RM_B_X + RM_B_P);    // [16 key][16 head][32]
    __bf16* const Vs = Ks + RM_B_R / 2;
    float* const Cs = reinterpret_cast<float*>(rm_lds + RM_B_S + RM_B_X + RM_B_P + 2 * RM_B_R);   // [32 q][16 head]
    RM_PROLOGUE
    float ghi[RM_HF], glo[RM_HF];
    rel_freq_table<RM_HF>(freq, 0, lane, ghi, glo);
    const int pq = tid >> 4, pk = tid & 15;                    // the pair this thread forms s_ij of
    const float4 xi = rel_load_xt(xt, ldxt, min(r0 + pq, kend - 1));
    // per query: q' of queries 4 w + t, row = head li of the group
    bf16x8 qpf[4];
    f32x4 uu[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        qpf[t] = rm_ld8(qp + (long long)min(r0 + 4 * wave + t, kend - 1) * ldqp + min(head0 + li, H - 1) * RM_DH + 8 * g4);
        rm_zero(uu[t][0]); rm_zero(uu[t][1]);
    }
    // per head: q of heads 2 w + j, query groups qg of 16, column = query li
    bf16x8 qf[2][2];
    f32x4 o[2][2][2];
    float m[2][2], l[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            qf[j][qg] = rm_ld8(qkv + (long long)min(r0 + 16 * qg + li, kend - 1) * ld + min(head0 + 2 * wave + j, H - 1) * RM_DH + 8 * g4);
            rm_zero(o[j][qg][0]); rm_zero(o[j][qg][1]);
            m[j][qg] = -INFINITY; l[j][qg] = 0.0f;
        }
    bf16x8 kn[2], vn[2];
    rm_fetch(kn, qkv, ld, E, head0, H, kbeg, kend - 1, tid);
    rm_fetch(vn, qkv, ld, 2 * E, head0, H, kbeg, kend - 1, tid);
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + pk, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * RM_KB;
        __syncthreads();                                      // A: every wave is done with the previous block
        rm_put(Ks, kn, tid);
        rm_put(Vs, vn, tid);
        rm_produce(Ss + (pq * RM_KB + pk) * RM_DH, rel_pair_arg(xi, xk), ghi, glo);
        rm_fetch(kn, qkv, ld, E, head0, H, kb + RM_KB, kend - 1, tid);
        rm_fetch(vn, qkv, ld, 2 * E, head0, H, kb + RM_KB, kend - 1, tid);
        xk = rel_load_xt(xt, ldxt, min(kb + RM_KB + pk, kend - 1));
        __syncthreads();                                      // B: the block is complete
#pragma unroll
        for (int t = 0; t < 4; ++t) {                         // bias[head][key] of query 4 w + t, in the exp2 domain
            const int q = 4 * wave + t;
            f32x4 d;
            rm_zero(d);
            d = rm_mma32(qpf[t], rm_ld8(Ss + (q * RM_KB + li) * RM_DH + 8 * g4), d);
#pragma unroll
            for (int r = 0; r < 4; ++r) Xs[((4 * g4 + r) * RM_ROWS + q) * RM_KB + li] = d[r] * REL_LOG2E;
        }
        __syncthreads();                                      // C: the bias scores are in X
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j;
            const bf16x8 kf = rm_ld8(Ks + (li * RM_G + hl) * RM_DH + 8 * g4);
            const rm_s16x4 vt0 = rm_tr(Vs, RM_G * RM_DH, hl * RM_DH, lane), vt1 = rm_tr(Vs, RM_G * RM_DH, hl * RM_DH + 16, lane);
#pragma unroll
            for (int qg = 0; qg < 2; ++qg) {
                const int q = 16 * qg + li;
                f32x4 s;
                rm_zero(s);
                s = rm_mma32(kf, qf[j][qg], s);               // S^T[key 4 g4 + r][query li]
                const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RM_ROWS + q) * RM_KB + 4 * g4);
                float sc[4] = {fmaf(s[0], scale2, x.x), fmaf(s[1], scale2, x.y), fmaf(s[2], scale2, x.z), fmaf(s[3], scale2, x.w)};
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (kb + 4 * g4 + r >= kend) sc[r] = -INFINITY;
                float mx = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                const float mn = fmaxf(m[j][qg], mx);         // finite: key kb of every block exists
                const float corr = rm_exp2(m[j][qg] - mn);
                float p[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) p[r] = rm_exp2(sc[r] - mn);
                l[j][qg] = fmaf(l[j][qg], corr, (p[0] + p[1]) + (p[2] + p[3]));      // this lane's 4 keys; summed over g4 at the end
                m[j][qg] = mn;
                const rm_s16x4 pb = rm_pack4(p[0], p[1], p[2], p[3]);
                *reinterpret_cast<rm_s16x4*>(Ps + (q * RM_G + hl) * RM_KB + 4 * g4) = pb;
                if (g4 == 0) Cs[q * RM_G + hl] = corr;
#pragma unroll
                for (int r = 0; r < 4; ++r) { o[j][qg][0][r] *= corr; o[j][qg][1][r] *= corr; }
                o[j][qg][0] = rm_mma16(vt0, pb, o[j][qg][0]);    // O^T[d 16 n + 4 g4 + r][query li]
                o[j][qg][1] = rm_mma16(vt1, pb, o[j][qg][1]);
            }
        }
        __syncthreads();                                      // D: P and the rescale factors are in LDS
#pragma unroll
        for (int t = 0; t < 4; ++t) {                         // U_i[head 4 g4 + r][c 16 n + li] of query 4 w + t
            const int q = 4 * wave + t;
            const float4 c = *reinterpret_cast<const float4*>(Cs + q * RM_G + 4 * g4);
            const rm_s16x4 pa = *reinterpret_cast<const rm_s16x4*>(Ps + (q * RM_G + li) * RM_KB + 4 * g4);
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                uu[t][n][0] *= c.x; uu[t][n][1] *= c.y; uu[t][n][2] *= c.z; uu[t][n][3] *= c.w;
                uu[t][n] = rm_mma16(pa, rm_tr(Ss + q * RM_KB * RM_DH, RM_DH, 16 * n, lane), uu[t][n]);
            }
        }
    }
    __syncthreads();                                          // the last block's factors have been read
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int hl = 2 * wave + j, head = head0 + hl;
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            const int q = 16 * qg + li, qi = r0 + q;
            float lt = l[j][qg];
            lt += __shfl_xor(lt, 16);
            lt += __shfl_xor(lt, 32);
            const float inv = 1.0f / lt;
            if (g4 == 0) Cs[q * RM_G + hl] = inv;
            if (qi < kend && head < H) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    rm_store4(out + (long long)qi * ldo + head * RM_DH + 16 * n + 4 * g4, o[j][qg][n][0] * inv, o[j][qg][n][1] * inv,
                              o[j][qg][n][2] * inv, o[j][qg][n][3] * inv);
                if (g4 == 0) lse2[(long long)qi * H + head] = m[j][qg] + log2f(lt);
            }
        }
    }
    __syncthreads();                                          // 1 / l of every (query, head) is in LDS
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = 4 * wave + t, qi = r0 + q;
        const float4 c = *reinterpret_cast<const float4*>(Cs + q * RM_G + 4 * g4);
        const float inv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int head = head0 + 4 * g4 + r;
            if (qi < kend && head < H) {
                u[(long long)qi * ldu + head * RM_DH + li] = (__bf16)(uu[t][0][r] * inv[r]);
                u[(long long)qi * ldu + head * RM_DH + 16 + li] = (__bf16)(uu[t][1][r] * inv[r]);
            }
        }
    }
}

// dQ / dQ' pass: the workgroup owns 32 queries.  As the forward with two per-query products before the per-head step (bias and
// the bias part of dA) and dS in the place of P; scores are recomputed from lse2, nothing is rescaled.
__global__ __launch_bounds__(RM_NT) void rel_attn_mfma_bwd_dq_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const __bf16* __restrict__ dout, long long lddo,
    const __bf16* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    __bf16* __restrict__ dqkv, long long lddq, __bf16* __restrict__ dqp, long long lddqp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rm_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rm_lds);                               // [32 q][16 key][32]
    float* const Xs = reinterpret_cast<float*>(rm_lds + RM_B_S);                        // [16 head][32 q][16 key]: bias log2 e
    float* const Ys = reinterpret_cast<float*>(rm_lds + RM_B_S + RM_B_X);               // the same: dU_i . s_ij
    __bf16* const Ps = reinterpret_cast<__bf16*>(rm_lds + RM_B_S + 2 * RM_B_X);         // [32 q][16 head][16 key]: dS
    __bf16* const Ks = reinterpret_cast<__bf16*>(rm_lds + RM_B_S + 2 * RM_B_X + RM_B_P);
    __bf16* const Vs = Ks + RM_B_R / 2;
    RM_PROLOGUE
    float ghi[RM_HF], glo[RM_HF];
    rel_freq_table<RM_HF>(freq, 0, lane, ghi, glo);
    const int pq = tid >> 4, pk = tid & 15;
    const float4 xi = rel_load_xt(xt, ldxt, min(r0 + pq, kend - 1));
    const float scale2 = scale * REL_LOG2E;
    bf16x8 qpf[4], duf[4];
    f32x4 dqq[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long row = min(r0 + 4 * wave + t, kend - 1);
        const int col = min(head0 + li, H - 1) * RM_DH + 8 * g4;
        qpf[t] = rm_ld8(qp + row * ldqp + col);
        duf[t] = rm_ld8(du + row * lddu + col);
        rm_zero(dqq[t][0]); rm_zero(dqq[t][1]);
    }
    bf16x8 qf[2][2], gf[2][2];
    f32x4 dq[2][2][2];
    float ls[2][2], dl[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            const long long row = min(r0 + 16 * qg + li, kend - 1);
            const int hc = min(head0 + 2 * wave + j, H - 1);
            qf[j][qg] = rm_ld8(qkv + row * ld + hc * RM_DH + 8 * g4);
            gf[j][qg] = rm_ld8(dout + row * lddo + hc * RM_DH + 8 * g4);
            ls[j][qg] = lse2[row * H + hc];
            dl[j][qg] = delta[row * H + hc];
            rm_zero(dq[j][qg][0]); rm_zero(dq[j][qg][1]);
        }
    bf16x8 kn[2], vn[2];
    rm_fetch(kn, qkv, ld, E, head0, H, kbeg, kend - 1, tid);
    rm_fetch(vn, qkv, ld, 2 * E, head0, H, kbeg, kend - 1, tid);
    float4 xk = rel_load_xt(xt, ldxt, min(kbeg + pk, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int kb = kbeg + b * RM_KB;
        __syncthreads();                                      // A
        rm_put(Ks, kn, tid);
        rm_put(Vs, vn, tid);
        rm_produce(Ss + (pq * RM_KB + pk) * RM_DH, rel_pair_arg(xi, xk), ghi, glo);
        rm_fetch(kn, qkv, ld, E, head0, H, kb + RM_KB, kend - 1, tid);
        rm_fetch(vn, qkv, ld, 2 * E, head0, H, kb + RM_KB, kend - 1, tid);
        xk = rel_load_xt(xt, ldxt, min(kb + RM_KB + pk, kend - 1));
        __syncthreads();                                      // B
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = 4 * wave + t;
            const bf16x8 sf = rm_ld8(Ss + (q * RM_KB + li) * RM_DH + 8 * g4);
            f32x4 d, g;
            rm_zero(d); rm_zero(g);
            d = rm_mma32(qpf[t], sf, d);
            g = rm_mma32(duf[t], sf, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Xs[((4 * g4 + r) * RM_ROWS + q) * RM_KB + li] = d[r] * REL_LOG2E;
                Ys[((4 * g4 + r) * RM_ROWS + q) * RM_KB + li] = g[r];
            }
        }
        __syncthreads();                                      // C
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j;
            const bf16x8 kf = rm_ld8(Ks + (li * RM_G + hl) * RM_DH + 8 * g4);
            const bf16x8 vf = rm_ld8(Vs + (li * RM_G + hl) * RM_DH + 8 * g4);
            const rm_s16x4 kt0 = rm_tr(Ks, RM_G * RM_DH, hl * RM_DH, lane), kt1 = rm_tr(Ks, RM_G * RM_DH, hl * RM_DH + 16, lane);
#pragma unroll
            for (int qg = 0; qg < 2; ++qg) {
                const int q = 16 * qg + li;
                f32x4 s, dp;
                rm_zero(s); rm_zero(dp);
                s = rm_mma32(kf, qf[j][qg], s);               // S^T[key 4 g4 + r][query li]
                dp = rm_mma32(vf, gf[j][qg], dp);             // (dO . v)^T
                const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RM_ROWS + q) * RM_KB + 4 * g4);
                const float4 y = *reinterpret_cast<const float4*>(Ys + (hl * RM_ROWS + q) * RM_KB + 4 * g4);
                const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
                float dS[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float p = rm_exp2(fmaf(s[r], scale2, xs[r]) - ls[j][qg]);
                    if (kb + 4 * g4 + r >= kend) p = 0.0f;
                    dS[r] = p * ((dp[r] + ys[r]) - dl[j][qg]);
                }
                const rm_s16x4 db = rm_pack4(dS[0], dS[1], dS[2], dS[3]);
                *reinterpret_cast<rm_s16x4*>(Ps + (q * RM_G + hl) * RM_KB + 4 * g4) = db;
                dq[j][qg][0] = rm_mma16(kt0, db, dq[j][qg][0]);  // dq^T[d 16 n + 4 g4 + r][query li]
                dq[j][qg][1] = rm_mma16(kt1, db, dq[j][qg][1]);
            }
        }
        __syncthreads();                                      // D
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = 4 * wave + t;
            const rm_s16x4 pa = *reinterpret_cast<const rm_s16x4*>(Ps + (q * RM_G + li) * RM_KB + 4 * g4);
#pragma unroll
            for (int n = 0; n < 2; ++n) dqq[t][n] = rm_mma16(pa, rm_tr(Ss + q * RM_KB * RM_DH, RM_DH, 16 * n, lane), dqq[t][n]);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int head = head0 + 2 * wave + j;
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) {
            const int qi = r0 + 16 * qg + li;
            if (qi < kend && head < H) {
#pragma unroll
                for (int n = 0; n < 2; ++n)
                    rm_store4(dqkv + (long long)qi * lddq + head * RM_DH + 16 * n + 4 * g4, dq[j][qg][n][0] * scale,
                              dq[j][qg][n][1] * scale, dq[j][qg][n][2] * scale, dq[j][qg][n][3] * scale);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qi = r0 + 4 * wave + t;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int head = head0 + 4 * g4 + r;
            if (qi < kend && head < H) {
                dqp[(long long)qi * lddqp + head * RM_DH + li] = (__bf16)dqq[t][0][r];
                dqp[(long long)qi * lddqp + head * RM_DH + 16 + li] = (__bf16)dqq[t][1][r];
            }
        }
    }
}

// dK / dV pass: the workgroup owns 32 keys; the event's queries pass 16 at a time.  Per query (wave w: queries 2 w, 2 w + 1 of
// the block) bias and dU . s for the 32 keys; per head S = Q K^T and dP = dO V^T with the queries as rows, so that P and dS
// leave their accumulators as the B operands (k = query) of dv^T += dO^T P and dk^T += Q^T dS.
__global__ __launch_bounds__(RM_NT) void rel_attn_mfma_bwd_dkv_kernel(
    const __bf16* __restrict__ qkv, long long ld, const __bf16* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const __bf16* __restrict__ dout, long long lddo,
    const __bf16* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    __bf16* __restrict__ dqkv, long long lddq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rm_lds[];
    __bf16* const Ss = reinterpret_cast<__bf16*>(rm_lds);                               // [16 q][32 key][32]
    float* const Xs = reinterpret_cast<float*>(rm_lds + RM_B_S);                        // [16 head][32 key][16 q]: bias log2 e
    float* const Ys = reinterpret_cast<float*>(rm_lds + RM_B_S + RM_B_X);               // the same: dU_i . s_ij
    __bf16* const Qs = reinterpret_cast<__bf16*>(rm_lds + RM_B_S + 2 * RM_B_X);         // [16 q][16 head][32]
    __bf16* const Gs = Qs + RM_B_R / 2;                                                 // the same: dO
    float* const Ls = reinterpret_cast<float*>(rm_lds + RM_B_S + 2 * RM_B_X + 2 * RM_B_R);   // [16 q][16 head]
    float* const Ds = Ls + RM_KB * RM_G;
    RM_PROLOGUE
    float ghi[RM_HF], glo[RM_HF];
    rel_freq_table<RM_HF>(freq, 0, lane, ghi, glo);
    const int pq = tid >> 5, pk = tid & 31;                    // the pair this thread forms s_ij of: query of the block, key
    const float4 xj = rel_load_xt(xt, ldxt, min(r0 + pk, kend - 1));
    const float scale2 = scale * REL_LOG2E;
    const int hq = min(head0 + li, H - 1) * RM_DH + 8 * g4;    // per query: this lane's piece of q' and dU
    // per head: k, v of heads 2 w + j, key groups kg of 16, column = key li
    bf16x8 kf[2][2], vf[2][2];
    f32x4 dk[2][2][2], dv[2][2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            const long long row = min(r0 + 16 * kg + li, kend - 1);
            const int hc = min(head0 + 2 * wave + j, H - 1);
            kf[j][kg] = rm_ld8(qkv + row * ld + E + hc * RM_DH + 8 * g4);
            vf[j][kg] = rm_ld8(qkv + row * ld + 2 * E + hc * RM_DH + 8 * g4);
            rm_zero(dk[j][kg][0]); rm_zero(dk[j][kg][1]); rm_zero(dv[j][kg][0]); rm_zero(dv[j][kg][1]);
        }
    // lse2 / delta of (query tid / 16, head tid % 16) of the block, by the first 256 threads (the others load the same again)
    const int sq = (tid >> 4) & 15, sh = min(head0 + (tid & 15), H - 1);
    bf16x8 qn[2], gn_[2], qpn[2], dun[2];
    float ln, dn;
    rm_fetch(qn, qkv, ld, 0, head0, H, kbeg, kend - 1, tid);
    rm_fetch(gn_, dout, lddo, 0, head0, H, kbeg, kend - 1, tid);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long long row = min(kbeg + 2 * wave + t, kend - 1);
        qpn[t] = rm_ld8(qp + row * ldqp + hq);
        dun[t] = rm_ld8(du + row * lddu + hq);
    }
    ln = lse2[(long long)min(kbeg + sq, kend - 1) * H + sh];
    dn = delta[(long long)min(kbeg + sq, kend - 1) * H + sh];
    float4 xq = rel_load_xt(xt, ldxt, min(kbeg + pq, kend - 1));
    for (int b = 0; b < nb; ++b) {
        const int qb = kbeg + b * RM_KB;
        __syncthreads();                                      // A
        rm_put(Qs, qn, tid);
        rm_put(Gs, gn_, tid);
        if (tid < RM_KB * RM_G) { Ls[tid] = ln; Ds[tid] = dn; }
        rm_produce(Ss + (pq * RM_ROWS + pk) * RM_DH, rel_pair_arg(xq, xj), ghi, glo);      // query - key
        bf16x8 qpf[2], duf[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) { qpf[t] = qpn[t]; duf[t] = dun[t]; }
        rm_fetch(qn, qkv, ld, 0, head0, H, qb + RM_KB, kend - 1, tid);
        rm_fetch(gn_, dout, lddo, 0, head0, H, qb + RM_KB, kend - 1, tid);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long row = min(qb + RM_KB + 2 * wave + t, kend - 1);
            qpn[t] = rm_ld8(qp + row * ldqp + hq);
            dun[t] = rm_ld8(du + row * lddu + hq);
        }
        ln = lse2[(long long)min(qb + RM_KB + sq, kend - 1) * H + sh];
        dn = delta[(long long)min(qb + RM_KB + sq, kend - 1) * H + sh];
        xq = rel_load_xt(xt, ldxt, min(qb + RM_KB + pq, kend - 1));
        __syncthreads();                                      // B
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int q = 2 * wave + t;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const bf16x8 sf = rm_ld8(Ss + (q * RM_ROWS + 16 * kh + li) * RM_DH + 8 * g4);
                f32x4 d, g;
                rm_zero(d); rm_zero(g);
                d = rm_mma32(qpf[t], sf, d);                  // [head 4 g4 + r][key 16 kh + li]
                g = rm_mma32(duf[t], sf, g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    Xs[((4 * g4 + r) * RM_ROWS + 16 * kh + li) * RM_KB + q] = d[r] * REL_LOG2E;
                    Ys[((4 * g4 + r) * RM_ROWS + 16 * kh + li) * RM_KB + q] = g[r];
                }
            }
        }
        __syncthreads();                                      // C
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int hl = 2 * wave + j;
            const bf16x8 qa = rm_ld8(Qs + (li * RM_G + hl) * RM_DH + 8 * g4);
            const bf16x8 ga = rm_ld8(Gs + (li * RM_G + hl) * RM_DH + 8 * g4);
            const rm_s16x4 qt0 = rm_tr(Qs, RM_G * RM_DH, hl * RM_DH, lane), qt1 = rm_tr(Qs, RM_G * RM_DH, hl * RM_DH + 16, lane);
            const rm_s16x4 gt0 = rm_tr(Gs, RM_G * RM_DH, hl * RM_DH, lane), gt1 = rm_tr(Gs, RM_G * RM_DH, hl * RM_DH + 16, lane);
            float Lr[4], Dr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { Lr[r] = Ls[(4 * g4 + r) * RM_G + hl]; Dr[r] = Ds[(4 * g4 + r) * RM_G + hl]; }
#pragma unroll
            for (int kg = 0; kg < 2; ++kg) {
                f32x4 s, dp;
                rm_zero(s); rm_zero(dp);
                s = rm_mma32(qa, kf[j][kg], s);               // S[query 4 g4 + r][key li]
                dp = rm_mma32(ga, vf[j][kg], dp);
                const float4 x = *reinterpret_cast<const float4*>(Xs + (hl * RM_ROWS + 16 * kg + li) * RM_KB + 4 * g4);
                const float4 y = *reinterpret_cast<const float4*>(Ys + (hl * RM_ROWS + 16 * kg + li) * RM_KB + 4 * g4);
                const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
                float p[4], dS[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = rm_exp2(fmaf(s[r], scale2, xs[r]) - Lr[r]);
                    if (qb + 4 * g4 + r >= kend) p[r] = 0.0f;
                    dS[r] = p[r] * ((dp[r] + ys[r]) - Dr[r]);
                }
                const rm_s16x4 pb = rm_pack4(p[0], p[1], p[2], p[3]), db = rm_pack4(dS[0], dS[1], dS[2], dS[3]);
                dv[j][kg][0] = rm_mma16(gt0, pb, dv[j][kg][0]);  // dv^T[d 16 n + 4 g4 + r][key li]
                dv[j][kg][1] = rm_mma16(gt1, pb, dv[j][kg][1]);
                dk[j][kg][0] = rm_mma16(qt0, db, dk[j][kg][0]);
                dk[j][kg][1] = rm_mma16(qt1, db, dk[j][kg][1]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int head = head0 + 2 * wave + j;
#pragma unroll
        for (int kg = 0; kg < 2; ++kg) {
            const int kj = r0 + 16 * kg + li;
            if (kj < kend && head < H) {
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    rm_store4(dqkv + (long long)kj * lddq + E + head * RM_DH + 16 * n + 4 * g4, dk[j][kg][n][0] * scale,
                              dk[j][kg][n][1] * scale, dk[j][kg][n][2] * scale, dk[j][kg][n][3] * scale);
                    rm_store4(dqkv + (long long)kj * lddq + 2 * E + head * RM_DH + 16 * n + 4 * g4, dv[j][kg][n][0], dv[j][kg][n][1],
                              dv[j][kg][n][2], dv[j][kg][n][3]);
                }
            }
        }
    }
}
#undef RM_PROLOGUE

bool rel_attn_mfma_supported(int DH) { return DH == RM_DH; }

hipError_t launch_rel_attn_mfma_fwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt, long long ldxt,
                                    const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N, void* out,
                                    long long ldo, void* u, long long ldu, float* lse2, hipStream_t st) {
    if (!rel_attn_mfma_supported(DH) || !rel_args_ok(false, 8, H, DH, ld, ldqp, ldxt, ldo, ldu)) return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once = rel_allow_lds(&rel_attn_mfma_fwd_kernel, RM_LDS_FWD);
    if (once != hipSuccess) return once;
    const dim3 grid(2u * (unsigned)(N / REL_TILE + B), (unsigned)((H + RM_G - 1) / RM_G)), block(RM_NT);
    hipLaunchKernelGGL(rel_attn_mfma_fwd_kernel, grid, block, RM_LDS_FWD, st, static_cast<const __bf16*>(qkv), ld,
                       static_cast<const __bf16*>(qp), ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B, rel_scale2(DH),
                       static_cast<__bf16*>(out), ldo, static_cast<__bf16*>(u), ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_mfma_bwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt, long long ldxt,
                                    const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N,
                                    const void* out, long long ldo, const void* u, long long ldu, const void* dout, long long lddo,
                                    const void* du, long long lddu, const float* lse2, float* delta, void* dqkv, long long lddq,
                                    void* dqp, long long lddqp, hipStream_t st) {
    if (!rel_attn_mfma_supported(DH) || !rel_args_ok(true, 8, H, DH, ld, ldqp, ldxt, ldo, ldu, lddo, lddu, lddq, lddqp))
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    static const hipError_t once_dq = rel_allow_lds(&rel_attn_mfma_bwd_dq_kernel, RM_LDS_DQ);
    static const hipError_t once_kv = rel_allow_lds(&rel_attn_mfma_bwd_dkv_kernel, RM_LDS_KV);
    if (once_dq != hipSuccess) return once_dq;
    if (once_kv != hipSuccess) return once_kv;
    const __bf16* qkv_ = static_cast<const __bf16*>(qkv);
    const __bf16* qp_ = static_cast<const __bf16*>(qp);
    const __bf16* dout_ = static_cast<const __bf16*>(dout);
    const __bf16* du_ = static_cast<const __bf16*>(du);
    const long long NH = (long long)N * H;
    hipLaunchKernelGGL(rel_attn_mfma_delta_kernel<RM_DH>, dim3((unsigned)((NH + 255) / 256)), dim3(256), 0, st,
                       static_cast<const __bf16*>(out), ldo, static_cast<const __bf16*>(u), ldu, dout_, lddo, du_, lddu, H, NH, delta);
    const dim3 grid(2u * (unsigned)(N / REL_TILE + B), (unsigned)((H + RM_G - 1) / RM_G)), block(RM_NT);
    const float scale = rel_scale(DH);
    hipLaunchKernelGGL(rel_attn_mfma_bwd_dq_kernel, grid, block, RM_LDS_DQ, st, qkv_, ld, qp_, ldqp, xt, ldxt, freq, H, ptr, tile_ptr,
                       B, scale, dout_, lddo, du_, lddu, lse2, delta, static_cast<__bf16*>(dqkv), lddq, static_cast<__bf16*>(dqp), lddqp);
    hipLaunchKernelGGL(rel_attn_mfma_bwd_dkv_kernel, grid, block, RM_LDS_KV, st, qkv_, ld, qp_, ldqp, xt, ldxt, freq, H, ptr,
                       tile_ptr, B, scale, dout_, lddo, du_, lddu, lse2, delta, static_cast<__bf16*>(dqkv), lddq);
    return hipGetLastError();
}

}  // namespace gn
