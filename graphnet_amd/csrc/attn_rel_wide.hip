// graphnet_amd/csrc/attn_rel_wide.hip — the spacetime-bias attention of attn_rel.hip for head width 64 (the IceMix B_d64
// shapes: hidden 768, 12 heads of 64).  Same mathematics, same pair-argument contract (attn_rel.hpp), another work split:
// with one lane per query the dQ pass would hold six 64-wide row vectors plus s_ij, 448 registers, and spill.  Here TWO
// lanes hold one query (forward, dQ pass) or one key (dK / dV pass), each half of the head width.
//
// Work split.  One workgroup of 128 threads (two waves) per (64-row tile of the plan, head); wave w owns rows 32 w .. 32 w + 31
// of the tile; lanes l and l ^ 32 of a wave are the halves h = l / 32 of row 32 w + (l & 31).
//   row-side vectors (q, o, dO, dq; k, v, dk, dv):  half h owns columns [32 h, 32 h + 32) of the head
//   embedding side (q', U, dU, dq', s_ij):          half h owns frequencies [16 h, 16 h + 16), i.e. the sine columns
//                                                   16 h + k and the cosine columns 32 + 16 h + k, k < 16
// so a lane evaluates 16 sine / cosine pairs per pair of pulses, as at head width 32, and nothing is evaluated twice.
//
// Sums over the head width.  Every dot product (score, dA, delta) is a partial sum per half, inside a half in the order of
// attn_rel.hip: the bias terms first, ascending k with sine then cosine, then the q . k / dO . v terms in ascending column.
// The halves exchange their partials with v_permlane32_swap (register to register, no LDS) and both form half0 + half1 in
// that operand order: the two lanes of a row hold the same bits of the score, m, l, p and dS and take the same branch of
// the online softmax.  delta is summed exactly as dA, so a softmax over one key still has a gradient of exactly 0.
//
// LDS.  Forward and dQ pass: a 64-key tile of K and of V (2 x 16 KB) and the pulse columns (1 KB) are staged once per
// workgroup and read by both waves; a ds_read_b128 of a wave carries two broadcast addresses, one per half.  dK / dV pass:
// the event's queries stream through LDS 32 at a time (q, q', dO, dU: 4 x 8 KB, and lse2, delta, pulse columns).
// The frequency table (hi + lo of f_k / 2 pi, formed in double) differs between the halves of a wave and is held in
// registers, 32 per lane.  fp32 operands and accumulation, no atomics, a fixed summation order; no matrix instructions:
// the bias is 16 transcendental pairs per lane and key, and the fp32 contract forbids narrower operands.
#include "attn_rel.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int RW_DH = 64;                 // head width
constexpr int RW_HALF = 32;               // floats of every vector per lane
constexpr int RW_HF = 16;                 // frequencies per lane
constexpr int RW_THREADS = 128;
constexpr int RW_QT = 32;                 // queries per LDS stage of the dK / dV pass

// hi + lo of f_k / 2 pi for the 16 frequencies of half h (the double arithmetic of rel_freq_table; the half differs between
// the lanes of a wave, so every lane forms its own table)
__device__ __forceinline__ void rw_freq_table(const float* __restrict__ freq, int half, float (&ghi)[RW_HF], float (&glo)[RW_HF]) {
#pragma unroll
    for (int k = 0; k < RW_HF; ++k) {
        const double g = (double)freq[RW_HF * half + k] * 0.15915494309189534561;
        ghi[k] = (float)g;
        glo[k] = (float)(g - (double)ghi[k]);
    }
}

static_assert(RW_HALF == 32 && RW_HF == 16, "rel_load_emb / rel_store_emb: 16 sine and 16 cosine columns per lane, 32 apart");

// thread -> row of the tile (wave w, lane l: 32 w + (l & 31)); the half is (lane >> 5) & 1
#define RW_PROLOGUE(ROW0, ROWI)                                                                                 \
    constexpr int DH = RW_DH;                                                                                   \
    REL_TILE_PROLOGUE_AT(ROW0, ROWI, (lane >> 6) * 32 + (lane & 31))                                            \
    const int half = (lane >> 5) & 1;                                                                           \
    const int crow = head * DH + RW_HALF * half;          /* first row-side column of this lane */              \
    const int cemb = head * DH + RW_HF * half;            /* first sine column; the cosines start 32 further */

__global__ __launch_bounds__(RW_THREADS) void rel_attn_wide_fwd_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, float* __restrict__ out, long long ldo,
    float* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    __shared__ float Ks[REL_TILE * RW_DH];
    __shared__ float Vs[REL_TILE * RW_DH];
    __shared__ float4 Xs[REL_TILE];
    RW_PROLOGUE(q0, qi)
    float ghi[RW_HF], glo[RW_HF];
    rw_freq_table(freq, half, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    float q[RW_HALF], qq[RW_HALF], o[RW_HALF], uu[RW_HALF];
    rel_load_row(q, qkv + (long long)myrow * ld + crow, scale2);
    rel_load_emb(qq, qp + (long long)myrow * ldqp + cemb, REL_LOG2E);
#pragma unroll
    for (int d = 0; d < RW_HALF; ++d) { o[d] = 0.0f; uu[d] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    for (int kt = kbeg; kt < kend; kt += REL_TILE) {
        __syncthreads();
        rel_stage<RW_DH, REL_TILE, RW_THREADS>(Ks, qkv, ld, E + head * DH, kt, kend - 1, lane);
        rel_stage<RW_DH, REL_TILE, RW_THREADS>(Vs, qkv, ld, 2 * E + head * DH, kt, kend - 1, lane);
        if (lane < REL_TILE) Xs[lane] = rel_load_xt(xt, ldxt, min(kt + lane, kend - 1));
        __syncthreads();
        const int nk = min(REL_TILE, kend - kt);
        for (int c = 0; c < nk; ++c) {
            const float a = rel_pair_arg(xi, Xs[c]);
            float sc[RW_HALF];
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < RW_HF; ++k) {
                rel_sincos(a, ghi[k], glo[k], sc[k], sc[RW_HF + k]);
                acc = fmaf(qq[k], sc[k], acc);
                acc = fmaf(qq[RW_HF + k], sc[RW_HF + k], acc);
            }
            const float* kr = Ks + c * RW_DH + RW_HALF * half;
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                acc = fmaf(q[4 * d4], kk.x, acc); acc = fmaf(q[4 * d4 + 1], kk.y, acc);
                acc = fmaf(q[4 * d4 + 2], kk.z, acc); acc = fmaf(q[4 * d4 + 3], kk.w, acc);
            }
            acc = rel_pair_sum(acc);                         // the score, the same bits on both halves
            if (acc > m) {                                  // a new maximum: rescale what has been summed so far
                const float corr = exp2f(m - acc);
                l *= corr;
#pragma unroll
                for (int d = 0; d < RW_HALF; ++d) { o[d] *= corr; uu[d] *= corr; }
                m = acc;
            }
            const float p = exp2f(acc - m);
            l += p;
            const float* vr = Vs + c * RW_DH + RW_HALF * half;
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                o[4 * d4] = fmaf(p, vv.x, o[4 * d4]); o[4 * d4 + 1] = fmaf(p, vv.y, o[4 * d4 + 1]);
                o[4 * d4 + 2] = fmaf(p, vv.z, o[4 * d4 + 2]); o[4 * d4 + 3] = fmaf(p, vv.w, o[4 * d4 + 3]);
            }
#pragma unroll
            for (int d = 0; d < RW_HALF; ++d) uu[d] = fmaf(p, sc[d], uu[d]);
        }
    }
    if (valid) {
        const float inv = 1.0f / l;
        rel_store_row(out + (long long)qi * ldo + crow, o, inv);
        rel_store_emb(u + (long long)qi * ldu + cemb, uu, inv);
        if (half == 0) lse2[(long long)qi * H + head] = m + log2f(l);
    }
}

// dQ / dQ' pass: two lanes = one query.  Also writes delta[i, h] = dO_i . O_i + dU_i . U_i for the dK / dV pass.
__global__ __launch_bounds__(RW_THREADS) void rel_attn_wide_bwd_dq_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ out, long long ldo,
    const float* __restrict__ u, long long ldu, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq, float* __restrict__ dqp, long long lddqp) {
    __shared__ float Ks[REL_TILE * RW_DH];
    __shared__ float Vs[REL_TILE * RW_DH];
    __shared__ float4 Xs[REL_TILE];
    RW_PROLOGUE(q0, qi)
    float ghi[RW_HF], glo[RW_HF];
    rw_freq_table(freq, half, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float q[RW_HALF], qq[RW_HALF], go[RW_HALF], gu[RW_HALF], dq[RW_HALF], dqq[RW_HALF];
    rel_load_row(q, qkv + (long long)myrow * ld + crow, scale2);
    rel_load_emb(qq, qp + (long long)myrow * ldqp + cemb, REL_LOG2E);
    rel_load_row(go, dout + (long long)myrow * lddo + crow, 1.0f);
    rel_load_emb(gu, du + (long long)myrow * lddu + cemb, 1.0f);
    float dl = 0.0f;
    {
        // delta = dU . U + dO . O, per half in the order in which dA = dU . s + dO . v is summed per key below, then the same
        // half0 + half1: with a single key (U = s, O = v bit for bit) dA - delta is exactly 0
        float t[RW_HALF];
        rel_load_emb(t, u + (long long)myrow * ldu + cemb, 1.0f);
#pragma unroll
        for (int k = 0; k < RW_HF; ++k) { dl = fmaf(gu[k], t[k], dl); dl = fmaf(gu[RW_HF + k], t[RW_HF + k], dl); }
        rel_load_row(t, out + (long long)myrow * ldo + crow, 1.0f);
#pragma unroll
        for (int d = 0; d < RW_HALF; ++d) dl = fmaf(go[d], t[d], dl);
        dl = rel_pair_sum(dl);
    }
#pragma unroll
    for (int d = 0; d < RW_HALF; ++d) { dq[d] = 0.0f; dqq[d] = 0.0f; }
    const float ls = lse2[(long long)myrow * H + head];
    for (int kt = kbeg; kt < kend; kt += REL_TILE) {
        __syncthreads();
        rel_stage<RW_DH, REL_TILE, RW_THREADS>(Ks, qkv, ld, E + head * DH, kt, kend - 1, lane);
        rel_stage<RW_DH, REL_TILE, RW_THREADS>(Vs, qkv, ld, 2 * E + head * DH, kt, kend - 1, lane);
        if (lane < REL_TILE) Xs[lane] = rel_load_xt(xt, ldxt, min(kt + lane, kend - 1));
        __syncthreads();
        const int nk = min(REL_TILE, kend - kt);
        for (int c = 0; c < nk; ++c) {
            const float a = rel_pair_arg(xi, Xs[c]);
            float sc[RW_HALF];
            float s = 0.0f, dp = 0.0f;
#pragma unroll
            for (int k = 0; k < RW_HF; ++k) {
                rel_sincos(a, ghi[k], glo[k], sc[k], sc[RW_HF + k]);
                s = fmaf(qq[k], sc[k], s); s = fmaf(qq[RW_HF + k], sc[RW_HF + k], s);
                dp = fmaf(gu[k], sc[k], dp); dp = fmaf(gu[RW_HF + k], sc[RW_HF + k], dp);
            }
            const float* kr = Ks + c * RW_DH + RW_HALF * half;
            const float* vr = Vs + c * RW_DH + RW_HALF * half;
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                s = fmaf(q[4 * d4], kk.x, s); s = fmaf(q[4 * d4 + 1], kk.y, s);
                s = fmaf(q[4 * d4 + 2], kk.z, s); s = fmaf(q[4 * d4 + 3], kk.w, s);
                dp = fmaf(go[4 * d4], vv.x, dp); dp = fmaf(go[4 * d4 + 1], vv.y, dp);
                dp = fmaf(go[4 * d4 + 2], vv.z, dp); dp = fmaf(go[4 * d4 + 3], vv.w, dp);
            }
            s = rel_pair_sum(s);
            dp = rel_pair_sum(dp);
            const float dS = exp2f(s - ls) * (dp - dl);
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                dq[4 * d4] = fmaf(dS, kk.x, dq[4 * d4]); dq[4 * d4 + 1] = fmaf(dS, kk.y, dq[4 * d4 + 1]);
                dq[4 * d4 + 2] = fmaf(dS, kk.z, dq[4 * d4 + 2]); dq[4 * d4 + 3] = fmaf(dS, kk.w, dq[4 * d4 + 3]);
            }
#pragma unroll
            for (int d = 0; d < RW_HALF; ++d) dqq[d] = fmaf(dS, sc[d], dqq[d]);
        }
    }
    if (valid) {
        rel_store_row(dqkv + (long long)qi * lddq + crow, dq, scale);
        rel_store_emb(dqp + (long long)qi * lddqp + cemb, dqq, 1.0f);
        if (half == 0) delta[(long long)qi * H + head] = dl;
    }
}

// dK / dV pass: two lanes = one key; the event's queries (q, q', dO, dU, lse2, delta, pulse columns) stream through LDS,
// RW_QT at a time, and every lane reads its half of each of them.
__global__ __launch_bounds__(RW_THREADS) void rel_attn_wide_bwd_dkv_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq) {
    __shared__ float Qs[RW_QT * RW_DH];
    __shared__ float Ps[RW_QT * RW_DH];
    __shared__ float Gs[RW_QT * RW_DH];
    __shared__ float Us[RW_QT * RW_DH];
    __shared__ float Ls[RW_QT];
    __shared__ float Ds[RW_QT];
    __shared__ float4 Xs[RW_QT];
    RW_PROLOGUE(k0, kj)
    float ghi[RW_HF], glo[RW_HF];
    rw_freq_table(freq, half, ghi, glo);
    const float4 xj = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float k[RW_HALF], v[RW_HALF], dk[RW_HALF], dv[RW_HALF];
    rel_load_row(k, qkv + (long long)myrow * ld + E + crow, scale2);
    rel_load_row(v, qkv + (long long)myrow * ld + 2 * E + crow, 1.0f);
#pragma unroll
    for (int d = 0; d < RW_HALF; ++d) { dk[d] = 0.0f; dv[d] = 0.0f; }
    for (int qt = kbeg; qt < kend; qt += RW_QT) {
        __syncthreads();
        rel_stage<RW_DH, RW_QT, RW_THREADS>(Qs, qkv, ld, head * DH, qt, kend - 1, lane);
        rel_stage<RW_DH, RW_QT, RW_THREADS>(Ps, qp, ldqp, head * DH, qt, kend - 1, lane);
        rel_stage<RW_DH, RW_QT, RW_THREADS>(Gs, dout, lddo, head * DH, qt, kend - 1, lane);
        rel_stage<RW_DH, RW_QT, RW_THREADS>(Us, du, lddu, head * DH, qt, kend - 1, lane);
        if (lane < RW_QT) {
            const int row = min(qt + lane, kend - 1);
            Ls[lane] = lse2[(long long)row * H + head];
            Ds[lane] = delta[(long long)row * H + head];
            Xs[lane] = rel_load_xt(xt, ldxt, row);
        }
        __syncthreads();
        const int nq = min(RW_QT, kend - qt);
        for (int c = 0; c < nq; ++c) {
            const float a = rel_pair_arg(Xs[c], xj);                  // query - key, as in the other two kernels
            const float* qr = Qs + c * RW_DH + RW_HALF * half;
            const float* gr = Gs + c * RW_DH + RW_HALF * half;
            const float* pr = Ps + c * RW_DH + RW_HF * half;          // sines; the cosines 32 further
            const float* ur = Us + c * RW_DH + RW_HF * half;
            float bias = 0.0f, dp = 0.0f;
#pragma unroll
            for (int kk = 0; kk < RW_HF; ++kk) {
                float sn, cs;
                rel_sincos(a, ghi[kk], glo[kk], sn, cs);
                bias = fmaf(pr[kk], sn, bias); bias = fmaf(pr[32 + kk], cs, bias);
                dp = fmaf(ur[kk], sn, dp); dp = fmaf(ur[32 + kk], cs, dp);
            }
            float s = bias * REL_LOG2E;
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                s = fmaf(k[4 * d4], qv.x, s); s = fmaf(k[4 * d4 + 1], qv.y, s);
                s = fmaf(k[4 * d4 + 2], qv.z, s); s = fmaf(k[4 * d4 + 3], qv.w, s);
                dp = fmaf(v[4 * d4], gg.x, dp); dp = fmaf(v[4 * d4 + 1], gg.y, dp);
                dp = fmaf(v[4 * d4 + 2], gg.z, dp); dp = fmaf(v[4 * d4 + 3], gg.w, dp);
            }
            s = rel_pair_sum(s);
            dp = rel_pair_sum(dp);
            const float p = exp2f(s - Ls[c]);
            const float dS = p * (dp - Ds[c]);
#pragma unroll
            for (int d4 = 0; d4 < RW_HALF / 4; ++d4) {
                const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                dv[4 * d4] = fmaf(p, gg.x, dv[4 * d4]); dv[4 * d4 + 1] = fmaf(p, gg.y, dv[4 * d4 + 1]);
                dv[4 * d4 + 2] = fmaf(p, gg.z, dv[4 * d4 + 2]); dv[4 * d4 + 3] = fmaf(p, gg.w, dv[4 * d4 + 3]);
                dk[4 * d4] = fmaf(dS, qv.x, dk[4 * d4]); dk[4 * d4 + 1] = fmaf(dS, qv.y, dk[4 * d4 + 1]);
                dk[4 * d4 + 2] = fmaf(dS, qv.z, dk[4 * d4 + 2]); dk[4 * d4 + 3] = fmaf(dS, qv.w, dk[4 * d4 + 3]);
            }
        }
    }
    if (valid) {
        rel_store_row(dqkv + (long long)kj * lddq + E + crow, dk, scale);
        rel_store_row(dqkv + (long long)kj * lddq + 2 * E + crow, dv, 1.0f);
    }
}
#undef RW_PROLOGUE

bool rel_attn_wide_supported(int DH) { return DH == RW_DH; }

hipError_t launch_rel_attn_wide_fwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                    long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                    int N, void* out, long long ldo, void* u, long long ldu, float* lse2, hipStream_t st) {
    if (!rel_attn_wide_supported(DH) || !rel_args_ok(false, 4, H, DH, ld, ldqp, ldxt, ldo, ldu)) return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)H), block(RW_THREADS);
    hipLaunchKernelGGL(rel_attn_wide_fwd_kernel, grid, block, 0, st, (const float*)qkv, ld, (const float*)qp, ldqp, xt, ldxt, freq,
                       H, ptr, tile_ptr, B, rel_scale2(DH), (float*)out, ldo, (float*)u, ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_wide_bwd(const void* qkv, long long ld, const void* qp, long long ldqp, const float* xt,
                                    long long ldxt, const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B,
                                    int N, const void* out, long long ldo, const void* u, long long ldu, const void* dout,
                                    long long lddo, const void* du, long long lddu, const float* lse2, float* delta,
                                    void* dqkv, long long lddq, void* dqp, long long lddqp, hipStream_t st) {
    if (!rel_attn_wide_supported(DH) || !rel_args_ok(true, 4, H, DH, ld, ldqp, ldxt, ldo, ldu, lddo, lddu, lddq, lddqp))
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)H), block(RW_THREADS);
    const float scale = rel_scale(DH);
    hipLaunchKernelGGL(rel_attn_wide_bwd_dq_kernel, grid, block, 0, st, (const float*)qkv, ld, (const float*)qp, ldqp, xt, ldxt,
                       freq, H, ptr, tile_ptr, B, scale, (const float*)out, ldo, (const float*)u, ldu, (const float*)dout, lddo,
                       (const float*)du, lddu, lse2, delta, (float*)dqkv, lddq, (float*)dqp, lddqp);
    hipLaunchKernelGGL(rel_attn_wide_bwd_dkv_kernel, grid, block, 0, st, (const float*)qkv, ld, (const float*)qp, ldqp, xt, ldxt,
                       freq, H, ptr, tile_ptr, B, scale, (const float*)dout, lddo, (const float*)du, lddu, lse2, delta,
                       (float*)dqkv, lddq);
    return hipGetLastError();
}

}  // namespace gn
