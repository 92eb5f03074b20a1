// graphnet_amd/csrc/attn_rel.hip — ragged multi-head attention with the spacetime bias of DeepIce computed on the fly
// (reference models/components/layers.py:389-499 `Attention_rel` with the `SpacetimeEncoder` bias of
// components/embedding.py:139-175).  The reference forms R[b, i, j, :] = W s_ij + b (fp32, [B, L, L, dh]) and contracts it
// twice per layer.  Here neither that tensor nor any padding exists:
//   score   q~_ih . k_jh + q~_ih . R_ij  =  q~_ih . k_jh + (W^T q~_ih) . s_ij  (+ q~_ih . b: constant over j, drops out)
//   output  sum_j a_ihj (v_jh + R_ij)    =  O_ih + W U_ih + b,   U_ih = sum_j a_ihj s_ij
// so the kernel takes q, k, v and the per-row operand q' = W^T q~, recomputes s_ij per pair from the four pulse columns and
// returns O and U; W and b stay in ordinary GEMMs outside.  s_ij carries no gradient (the pulse features are data):
//   dA_ij = dO_i . v_j + dU_i . s_ij,  D_i = dO_i . O_i + dU_i . U_i,  dS_ij = a_ij (dA_ij - D_i),
//   dq_i = scale sum_j dS_ij k_j,  dq'_i = sum_j dS_ij s_ij,  dk_j = scale sum_i dS_ij q_i,  dv_j = sum_i a_ij dO_i.
//
// Layout: as the exact-fp32 kernels of attn.hip — one wave per (64-row tile of the plan, head), one lane = one query
// (forward, dQ pass) or one key (dK/dV pass), the other side streams through LDS as broadcast reads; fp32 operands and
// accumulation; no atomics, a fixed summation order (two runs agree bit for bit).  The online softmax rescales O and U
// only when a key raises the running maximum.
//
// Pair argument (a CONTRACT, include/graphnet_amd.h): fp32, every operation rounded on its own, in this order.
// s_ij = [sin(a f_k) | cos(a f_k)], k < dh/2, |a f_k| up to 4096 rad.  The argument is reduced in revolutions with a
// two-term product: g_k = f_k / 2 pi is formed in double from the fp32 table once per wave and split hi + lo; t = a g_hi,
// e = fma(a, g_hi, -t) + a g_lo, r = fract(t) + e, then sine / cosine of 2 pi r by quadrant and polynomial (rel_sincos).
// The reduced argument is good to ~1e-7 revolutions; a bare a f_k / 2 pi in fp32 is not (2e-4 rad at 652 revolutions).
#include "common.hpp"
#include "launchers.hpp"

namespace gn {

constexpr int REL_TILE = 64;
constexpr float REL_LOG2E = 1.4426950408889634f;

// event of tile `tile`: largest e with tile_ptr[e] <= tile  (wave-uniform; the plan of gn_attention_plan)
__device__ __forceinline__ int rel_event_of_tile(const int* __restrict__ tile_ptr, int B, int tile) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_ptr[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// stage rows [r0, r0 + ROWS) (clamped to r_last) x DH floats of column block `col0` into LDS [ROWS][DH]
template <int DH, int ROWS>
__device__ __forceinline__ void rel_stage(float* __restrict__ dst, const float* __restrict__ src, long long ld,
                                          int col0, int r0, int r_last, int lane) {
    constexpr int V4 = DH / 4;
#pragma unroll
    for (int it = 0; it < ROWS * V4 / 64; ++it) {
        const int idx = it * 64 + lane;
        const int r = idx / V4, c4 = idx % V4;
        const int row = min(r0 + r, r_last);
        const float4 v = *reinterpret_cast<const float4*>(src + (long long)row * ld + col0 + c4 * 4);
        *reinterpret_cast<float4*>(dst + r * DH + c4 * 4) = v;
    }
}

__device__ __forceinline__ float4 rel_load_xt(const float* __restrict__ xt, long long ldxt, int row) {
    const float* p = xt + (long long)row * ldxt;
    return make_float4(p[0], p[1], p[2], p[3]);
}

// a = 1024 clip(sign(ds) sqrt|ds|, -4, 4), ds = ((dx^2 + dy^2) + dz^2) - (18 dt)^2, differences query - key.
// No FMA contraction: near null separation a fused dx*dx + dy*dy changes the sign of ds.
__device__ __forceinline__ float rel_pair_arg(const float4 xi, const float4 xj) {
#pragma clang fp contract(off)
    const float dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
    const float dx2 = dx * dx, dy2 = dy * dy, dz2 = dz * dz;
    const float sp = (dx2 + dy2) + dz2;
    const float dt = (xi.w - xj.w) * 18.0f;
    const float dt2 = dt * dt;
    const float ds = sp - dt2;
    float d = sqrtf(fabsf(ds));                 // correctly rounded (the __fsqrt_rn intrinsic is the bare 1-ulp v_sqrt_f32)
    d = ds < 0.0f ? -d : d;
    d = fminf(fmaxf(d, -4.0f), 4.0f);
    return d * 1024.0f;
}

// frequencies in revolutions per unit, hi + lo, wave-uniform (lane k forms entry k in double, then it is broadcast)
template <int HF>
__device__ __forceinline__ void rel_freq_table(const float* __restrict__ freq, int lane, float (&ghi)[HF], float (&glo)[HF]) {
    float hi_l = 0.0f, lo_l = 0.0f;
    if (lane < HF) {
        const double g = (double)freq[lane] * 0.15915494309189534561;
        hi_l = (float)g;
        lo_l = (float)(g - (double)hi_l);
    }
#pragma unroll
    for (int k = 0; k < HF; ++k) {
        ghi[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hi_l), k));
        glo[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo_l), k));
    }
}

// sin and cos of 2 pi r: quadrant q = rint(4 r), y = r - q / 4 (exact), degree-7 / degree-8 polynomials on |2 pi y| <= pi / 4
// (3.8e-7 absolute against double over the whole argument range, checked on the host).
__device__ __forceinline__ void rel_sincos(float a, float ghi, float glo, float& sn, float& cs) {
    float t, e;
    {
#pragma clang fp contract(off)
        t = a * ghi;
    }
    e = fmaf(a, ghi, -t);
    e = fmaf(a, glo, e);
    const float r = __builtin_amdgcn_fractf(t) + e;            // revolutions, [0, 1] up to rounding
    const float q = rintf(4.0f * r);
    const float x = fmaf(q, -0.25f, r) * 6.28318530717958648f;
    const float z = x * x;
    float ps = fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = fmaf(ps, z, -1.6666654611e-1f);
    ps = fmaf(ps * z, x, x);
    float pc = fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = fmaf(pc, z, 4.166664568298827e-2f);
    pc = fmaf(pc * z, z, fmaf(-0.5f, z, 1.0f));
    const unsigned qi = (unsigned)(int)q;
    const bool swap = qi & 1u;
    const unsigned us = __builtin_bit_cast(unsigned, swap ? pc : ps) ^ ((qi & 2u) << 30);
    const unsigned uc = __builtin_bit_cast(unsigned, swap ? ps : pc) ^ (((qi + 1u) & 2u) << 30);
    sn = __builtin_bit_cast(float, us);
    cs = __builtin_bit_cast(float, uc);
}

#define REL_TILE_PROLOGUE(ROW0, ROWI)                                                                           \
    const int tile = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;                                         \
    if (tile >= tile_ptr[B]) return;                                                                            \
    const int es = rel_event_of_tile(tile_ptr, B, tile);                                                        \
    const int e = tile_ptr[B + 1 + es];                                                                         \
    const int kbeg = ptr[e], kend = ptr[e + 1];                                                                 \
    const int ROW0 = kbeg + (tile - tile_ptr[es]) * REL_TILE;                                                   \
    const int E = H * DH;                                                                                       \
    const int ROWI = ROW0 + lane;                                                                               \
    const bool valid = ROWI < kend;                                                                             \
    const int myrow = valid ? ROWI : kend - 1;

template <int DH>
__global__ __launch_bounds__(64) void rel_attn_fwd_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale2, float* __restrict__ out, long long ldo,
    float* __restrict__ u, long long ldu, float* __restrict__ lse2) {
    constexpr int HF = DH / 2;
    __shared__ float Ks[REL_TILE * DH];
    __shared__ float Vs[REL_TILE * DH];
    __shared__ float4 Xs[REL_TILE];
    REL_TILE_PROLOGUE(q0, qi)
    float ghi[HF], glo[HF];
    rel_freq_table<HF>(freq, lane, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    float q[DH], qq[DH], o[DH], uu[DH];
#pragma unroll
    for (int d4 = 0; d4 < DH / 4; ++d4) {
        const float4 v = *reinterpret_cast<const float4*>(qkv + (long long)myrow * ld + head * DH + d4 * 4);
        q[4 * d4] = v.x * scale2; q[4 * d4 + 1] = v.y * scale2; q[4 * d4 + 2] = v.z * scale2; q[4 * d4 + 3] = v.w * scale2;
        const float4 w = *reinterpret_cast<const float4*>(qp + (long long)myrow * ldqp + head * DH + d4 * 4);
        qq[4 * d4] = w.x * REL_LOG2E; qq[4 * d4 + 1] = w.y * REL_LOG2E; qq[4 * d4 + 2] = w.z * REL_LOG2E; qq[4 * d4 + 3] = w.w * REL_LOG2E;
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) { o[d] = 0.0f; uu[d] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    for (int kt = kbeg; kt < kend; kt += REL_TILE) {
        __syncthreads();
        rel_stage<DH, REL_TILE>(Ks, qkv, ld, E + head * DH, kt, kend - 1, lane);
        rel_stage<DH, REL_TILE>(Vs, qkv, ld, 2 * E + head * DH, kt, kend - 1, lane);
        Xs[lane] = rel_load_xt(xt, ldxt, min(kt + lane, kend - 1));
        __syncthreads();
        const int nk = min(REL_TILE, kend - kt);
        for (int c = 0; c < nk; ++c) {
            const float a = rel_pair_arg(xi, Xs[c]);
            float sc[DH];
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < HF; ++k) {
                rel_sincos(a, ghi[k], glo[k], sc[k], sc[HF + k]);
                acc = fmaf(qq[k], sc[k], acc);
                acc = fmaf(qq[HF + k], sc[HF + k], acc);
            }
            const float* kr = Ks + c * DH;
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                acc = fmaf(q[4 * d4], kk.x, acc); acc = fmaf(q[4 * d4 + 1], kk.y, acc);
                acc = fmaf(q[4 * d4 + 2], kk.z, acc); acc = fmaf(q[4 * d4 + 3], kk.w, acc);
            }
            if (acc > m) {                                  // a new maximum: rescale what has been summed so far
                const float corr = exp2f(m - acc);
                l *= corr;
#pragma unroll
                for (int d = 0; d < DH; ++d) { o[d] *= corr; uu[d] *= corr; }
                m = acc;
            }
            const float p = exp2f(acc - m);
            l += p;
            const float* vr = Vs + c * DH;
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
                const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                o[4 * d4] = fmaf(p, vv.x, o[4 * d4]); o[4 * d4 + 1] = fmaf(p, vv.y, o[4 * d4 + 1]);
                o[4 * d4 + 2] = fmaf(p, vv.z, o[4 * d4 + 2]); o[4 * d4 + 3] = fmaf(p, vv.w, o[4 * d4 + 3]);
            }
#pragma unroll
            for (int d = 0; d < DH; ++d) uu[d] = fmaf(p, sc[d], uu[d]);
        }
    }
    if (valid) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            *reinterpret_cast<float4*>(out + (long long)qi * ldo + head * DH + d4 * 4) =
                make_float4(o[4 * d4] * inv, o[4 * d4 + 1] * inv, o[4 * d4 + 2] * inv, o[4 * d4 + 3] * inv);
            *reinterpret_cast<float4*>(u + (long long)qi * ldu + head * DH + d4 * 4) =
                make_float4(uu[4 * d4] * inv, uu[4 * d4 + 1] * inv, uu[4 * d4 + 2] * inv, uu[4 * d4 + 3] * inv);
        }
        lse2[(long long)qi * H + head] = m + log2f(l);
    }
}

// dQ / dQ' pass: lane = query.  Also writes delta[i, h] = dO_i . O_i + dU_i . U_i for the dK / dV pass.
template <int DH>
__global__ __launch_bounds__(64) void rel_attn_bwd_dq_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ out, long long ldo,
    const float* __restrict__ u, long long ldu, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq, float* __restrict__ dqp, long long lddqp) {
    constexpr int HF = DH / 2;
    __shared__ float Ks[REL_TILE * DH];
    __shared__ float Vs[REL_TILE * DH];
    __shared__ float4 Xs[REL_TILE];
    REL_TILE_PROLOGUE(q0, qi)
    float ghi[HF], glo[HF];
    rel_freq_table<HF>(freq, lane, ghi, glo);
    const float4 xi = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float q[DH], qq[DH], go[DH], gu[DH], dq[DH], dqq[DH];
    float dl = 0.0f;
#pragma unroll
    for (int d4 = 0; d4 < DH / 4; ++d4) {
        const long long c = head * DH + d4 * 4;
        const float4 v = *reinterpret_cast<const float4*>(qkv + (long long)myrow * ld + c);
        q[4 * d4] = v.x * scale2; q[4 * d4 + 1] = v.y * scale2; q[4 * d4 + 2] = v.z * scale2; q[4 * d4 + 3] = v.w * scale2;
        const float4 w = *reinterpret_cast<const float4*>(qp + (long long)myrow * ldqp + c);
        qq[4 * d4] = w.x * REL_LOG2E; qq[4 * d4 + 1] = w.y * REL_LOG2E; qq[4 * d4 + 2] = w.z * REL_LOG2E; qq[4 * d4 + 3] = w.w * REL_LOG2E;
        const float4 g = *reinterpret_cast<const float4*>(dout + (long long)myrow * lddo + c);
        go[4 * d4] = g.x; go[4 * d4 + 1] = g.y; go[4 * d4 + 2] = g.z; go[4 * d4 + 3] = g.w;
        const float4 h = *reinterpret_cast<const float4*>(du + (long long)myrow * lddu + c);
        gu[4 * d4] = h.x; gu[4 * d4 + 1] = h.y; gu[4 * d4 + 2] = h.z; gu[4 * d4 + 3] = h.w;
    }
    {
        // delta = dU . U + dO . O, summed in the order in which dA = dU . s + dO . v is summed per key below: with a single
        // key (U = s, O = v bit for bit) dA - delta is then exactly 0, as the softmax of one score has no gradient
        float tu[DH];
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            const float4 uv = *reinterpret_cast<const float4*>(u + (long long)myrow * ldu + head * DH + d4 * 4);
            tu[4 * d4] = uv.x; tu[4 * d4 + 1] = uv.y; tu[4 * d4 + 2] = uv.z; tu[4 * d4 + 3] = uv.w;
        }
#pragma unroll
        for (int k = 0; k < HF; ++k) { dl = fmaf(gu[k], tu[k], dl); dl = fmaf(gu[HF + k], tu[HF + k], dl); }
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            const float4 ov = *reinterpret_cast<const float4*>(out + (long long)myrow * ldo + head * DH + d4 * 4);
            dl = fmaf(go[4 * d4], ov.x, dl); dl = fmaf(go[4 * d4 + 1], ov.y, dl);
            dl = fmaf(go[4 * d4 + 2], ov.z, dl); dl = fmaf(go[4 * d4 + 3], ov.w, dl);
        }
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) { dq[d] = 0.0f; dqq[d] = 0.0f; }
    const float ls = lse2[(long long)myrow * H + head];
    for (int kt = kbeg; kt < kend; kt += REL_TILE) {
        __syncthreads();
        rel_stage<DH, REL_TILE>(Ks, qkv, ld, E + head * DH, kt, kend - 1, lane);
        rel_stage<DH, REL_TILE>(Vs, qkv, ld, 2 * E + head * DH, kt, kend - 1, lane);
        Xs[lane] = rel_load_xt(xt, ldxt, min(kt + lane, kend - 1));
        __syncthreads();
        const int nk = min(REL_TILE, kend - kt);
        for (int c = 0; c < nk; ++c) {
            const float a = rel_pair_arg(xi, Xs[c]);
            float sc[DH];
            float s = 0.0f, dp = 0.0f;
#pragma unroll
            for (int k = 0; k < HF; ++k) {
                rel_sincos(a, ghi[k], glo[k], sc[k], sc[HF + k]);
                s = fmaf(qq[k], sc[k], s); s = fmaf(qq[HF + k], sc[HF + k], s);
                dp = fmaf(gu[k], sc[k], dp); dp = fmaf(gu[HF + k], sc[HF + k], dp);
            }
            const float* kr = Ks + c * DH;
            const float* vr = Vs + c * DH;
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                const float4 vv = *reinterpret_cast<const float4*>(vr + 4 * d4);
                s = fmaf(q[4 * d4], kk.x, s); s = fmaf(q[4 * d4 + 1], kk.y, s);
                s = fmaf(q[4 * d4 + 2], kk.z, s); s = fmaf(q[4 * d4 + 3], kk.w, s);
                dp = fmaf(go[4 * d4], vv.x, dp); dp = fmaf(go[4 * d4 + 1], vv.y, dp);
                dp = fmaf(go[4 * d4 + 2], vv.z, dp); dp = fmaf(go[4 * d4 + 3], vv.w, dp);
            }
            const float dS = exp2f(s - ls) * (dp - dl);
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
                const float4 kk = *reinterpret_cast<const float4*>(kr + 4 * d4);
                dq[4 * d4] = fmaf(dS, kk.x, dq[4 * d4]); dq[4 * d4 + 1] = fmaf(dS, kk.y, dq[4 * d4 + 1]);
                dq[4 * d4 + 2] = fmaf(dS, kk.z, dq[4 * d4 + 2]); dq[4 * d4 + 3] = fmaf(dS, kk.w, dq[4 * d4 + 3]);
            }
#pragma unroll
            for (int d = 0; d < DH; ++d) dqq[d] = fmaf(dS, sc[d], dqq[d]);
        }
    }
    if (valid) {
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            *reinterpret_cast<float4*>(dqkv + (long long)qi * lddq + head * DH + d4 * 4) =
                make_float4(dq[4 * d4] * scale, dq[4 * d4 + 1] * scale, dq[4 * d4 + 2] * scale, dq[4 * d4 + 3] * scale);
            *reinterpret_cast<float4*>(dqp + (long long)qi * lddqp + head * DH + d4 * 4) =
                make_float4(dqq[4 * d4], dqq[4 * d4 + 1], dqq[4 * d4 + 2], dqq[4 * d4 + 3]);
        }
        delta[(long long)qi * H + head] = dl;
    }
}

// dK / dV pass: lane = key; the event's queries (q, q', dO, dU, lse2, delta, pulse columns) stream through LDS, QT at a time.
template <int DH, int QT>
__global__ __launch_bounds__(64) void rel_attn_bwd_dkv_kernel(
    const float* __restrict__ qkv, long long ld, const float* __restrict__ qp, long long ldqp,
    const float* __restrict__ xt, long long ldxt, const float* __restrict__ freq, int H, const int* __restrict__ ptr,
    const int* __restrict__ tile_ptr, int B, float scale, const float* __restrict__ dout, long long lddo,
    const float* __restrict__ du, long long lddu, const float* __restrict__ lse2, const float* __restrict__ delta,
    float* __restrict__ dqkv, long long lddq) {
    constexpr int HF = DH / 2;
    __shared__ float Qs[QT * DH];
    __shared__ float Ps[QT * DH];
    __shared__ float Gs[QT * DH];
    __shared__ float Us[QT * DH];
    __shared__ float Ls[QT];
    __shared__ float Ds[QT];
    __shared__ float4 Xs[QT];
    REL_TILE_PROLOGUE(k0, kj)
    float ghi[HF], glo[HF];
    rel_freq_table<HF>(freq, lane, ghi, glo);
    const float4 xj = rel_load_xt(xt, ldxt, myrow);
    const float scale2 = scale * REL_LOG2E;
    float k[DH], v[DH], dk[DH], dv[DH];
#pragma unroll
    for (int d4 = 0; d4 < DH / 4; ++d4) {
        const float4 a = *reinterpret_cast<const float4*>(qkv + (long long)myrow * ld + E + head * DH + d4 * 4);
        k[4 * d4] = a.x * scale2; k[4 * d4 + 1] = a.y * scale2; k[4 * d4 + 2] = a.z * scale2; k[4 * d4 + 3] = a.w * scale2;
        const float4 b = *reinterpret_cast<const float4*>(qkv + (long long)myrow * ld + 2 * E + head * DH + d4 * 4);
        v[4 * d4] = b.x; v[4 * d4 + 1] = b.y; v[4 * d4 + 2] = b.z; v[4 * d4 + 3] = b.w;
    }
#pragma unroll
    for (int d = 0; d < DH; ++d) { dk[d] = 0.0f; dv[d] = 0.0f; }
    for (int qt = kbeg; qt < kend; qt += QT) {
        __syncthreads();
        rel_stage<DH, QT>(Qs, qkv, ld, head * DH, qt, kend - 1, lane);
        rel_stage<DH, QT>(Ps, qp, ldqp, head * DH, qt, kend - 1, lane);
        rel_stage<DH, QT>(Gs, dout, lddo, head * DH, qt, kend - 1, lane);
        rel_stage<DH, QT>(Us, du, lddu, head * DH, qt, kend - 1, lane);
        if (lane < QT) {
            const int row = min(qt + lane, kend - 1);
            Ls[lane] = lse2[(long long)row * H + head];
            Ds[lane] = delta[(long long)row * H + head];
            Xs[lane] = rel_load_xt(xt, ldxt, row);
        }
        __syncthreads();
        const int nq = min(QT, kend - qt);
        for (int c = 0; c < nq; ++c) {
            const float a = rel_pair_arg(Xs[c], xj);                  // query - key, as in the other two kernels
            const float* qr = Qs + c * DH;
            const float* pr = Ps + c * DH;
            const float* gr = Gs + c * DH;
            const float* ur = Us + c * DH;
            float bias = 0.0f, dp = 0.0f;
#pragma unroll
            for (int kk = 0; kk < HF; ++kk) {
                float sn, cs;
                rel_sincos(a, ghi[kk], glo[kk], sn, cs);
                bias = fmaf(pr[kk], sn, bias); bias = fmaf(pr[HF + kk], cs, bias);
                dp = fmaf(ur[kk], sn, dp); dp = fmaf(ur[HF + kk], cs, dp);
            }
            float s = bias * REL_LOG2E;
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
                const float4 qv = *reinterpret_cast<const float4*>(qr + 4 * d4);
                const float4 gg = *reinterpret_cast<const float4*>(gr + 4 * d4);
                s = fmaf(k[4 * d4], qv.x, s); s = fmaf(k[4 * d4 + 1], qv.y, s);
                s = fmaf(k[4 * d4 + 2], qv.z, s); s = fmaf(k[4 * d4 + 3], qv.w, s);
                dp = fmaf(v[4 * d4], gg.x, dp); dp = fmaf(v[4 * d4 + 1], gg.y, dp);
                dp = fmaf(v[4 * d4 + 2], gg.z, dp); dp = fmaf(v[4 * d4 + 3], gg.w, dp);
            }
            const float p = exp2f(s - Ls[c]);
            const float dS = p * (dp - Ds[c]);
#pragma unroll
            for (int d4 = 0; d4 < DH / 4; ++d4) {
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
#pragma unroll
        for (int d4 = 0; d4 < DH / 4; ++d4) {
            *reinterpret_cast<float4*>(dqkv + (long long)kj * lddq + E + head * DH + d4 * 4) =
                make_float4(dk[4 * d4] * scale, dk[4 * d4 + 1] * scale, dk[4 * d4 + 2] * scale, dk[4 * d4 + 3] * scale);
            *reinterpret_cast<float4*>(dqkv + (long long)kj * lddq + 2 * E + head * DH + d4 * 4) =
                make_float4(dv[4 * d4], dv[4 * d4 + 1], dv[4 * d4 + 2], dv[4 * d4 + 3]);
        }
    }
}
#undef REL_TILE_PROLOGUE

bool rel_attn_supported(int DH) { return DH == 32; }

hipError_t launch_rel_attn_fwd(const float* qkv, long long ld, const float* qp, long long ldqp, const float* xt, long long ldxt,
                               const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N,
                               float* out, long long ldo, float* u, long long ldu, float* lse2, hipStream_t st) {
    if (!rel_attn_supported(DH) || ld % 4 || ldqp % 4 || ldo % 4 || ldu % 4 || ldxt < 4 || ld < 3ll * H * DH ||
        ldqp < (long long)H * DH || ldo < (long long)H * DH || ldu < (long long)H * DH)
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)H), block(REL_TILE);
    const float scale2 = REL_LOG2E / sqrtf((float)DH);
    hipLaunchKernelGGL((rel_attn_fwd_kernel<32>), grid, block, 0, st, qkv, ld, qp, ldqp, xt, ldxt, freq, H, ptr, tile_ptr, B,
                       scale2, out, ldo, u, ldu, lse2);
    return hipGetLastError();
}

hipError_t launch_rel_attn_bwd(const float* qkv, long long ld, const float* qp, long long ldqp, const float* xt, long long ldxt,
                               const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N,
                               const float* out, long long ldo, const float* u, long long ldu, const float* dout,
                               long long lddo, const float* du, long long lddu, const float* lse2, float* delta,
                               float* dqkv, long long lddq, float* dqp, long long lddqp, hipStream_t st) {
    const long long d = (long long)H * DH;
    if (!rel_attn_supported(DH) || ld % 4 || ldqp % 4 || ldo % 4 || ldu % 4 || lddo % 4 || lddu % 4 || lddq % 4 || lddqp % 4 ||
        ldxt < 4 || ld < 3 * d || lddq < 3 * d || ldqp < d || ldo < d || ldu < d || lddo < d || lddu < d || lddqp < d)
        return hipErrorInvalidValue;
    if (N == 0 || B == 0) return hipSuccess;
    const dim3 grid((unsigned)(N / REL_TILE + B), (unsigned)H), block(REL_TILE);
    const float scale = 1.0f / sqrtf((float)DH);
    // (the templates are written for any even DH; at DH = 64 the dQ pass holds six row vectors and s_ij, 448 registers,
    //  and spills - only 32 is instantiated, see rel_attn_supported)
    hipLaunchKernelGGL((rel_attn_bwd_dq_kernel<32>), grid, block, 0, st, qkv, ld, qp, ldqp, xt, ldxt, freq, H, ptr, tile_ptr,
                       B, scale, out, ldo, u, ldu, dout, lddo, du, lddu, lse2, delta, dqkv, lddq, dqp, lddqp);
    hipLaunchKernelGGL((rel_attn_bwd_dkv_kernel<32, REL_TILE>), grid, block, 0, st, qkv, ld, qp, ldqp, xt, ldxt, freq, H, ptr,
                       tile_ptr, B, scale, dout, lddo, du, lddu, lse2, delta, dqkv, lddq);
    return hipGetLastError();
}

}  // namespace gn
