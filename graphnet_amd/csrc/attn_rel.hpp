// graphnet_amd/csrc/attn_rel.hpp — what the six kernel families of the spacetime-bias attention share (attn_rel*.hip): the
// pair argument with its sine / cosine and the hi / lo frequency table (a CONTRACT, include/graphnet_amd.h), the event lookup
// over the plan of gn_attention_plan, LDS staging, the row and s_ij helpers of the fp32 families, and the host-side argument
// check, LDS opt-in and score scales of every launcher.  The matrix-core helpers are in attn_rel_mfma.hpp.
#pragma once
#include "common.hpp"
#include <cmath>

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

// stage rows [r0, r0 + ROWS) (clamped to r_last) x DH floats of column block `col0` into LDS [ROWS][DH], NT threads
template <int DH, int ROWS, int NT = 64>
__device__ __forceinline__ void rel_stage(float* __restrict__ dst, const float* __restrict__ src, long long ld,
                                          int col0, int r0, int r_last, int lane) {
    constexpr int V4 = DH / 4;
#pragma unroll
    for (int it = 0; it < ROWS * V4 / NT; ++it) {
        const int idx = it * NT + lane;
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

// frequencies [HF fb, HF fb + HF), block fb of the table, in revolutions per unit, hi + lo, wave-uniform (lane k forms entry k in
// double, then it is broadcast)
template <int HF>
__device__ __forceinline__ void rel_freq_table(const float* __restrict__ freq, int fb, int lane, float (&ghi)[HF], float (&glo)[HF]) {
    float hi_l = 0.0f, lo_l = 0.0f;
    if (lane < HF) {
        const double g = (double)freq[HF * fb + lane] * 0.15915494309189534561;
        hi_l = (float)g;
        lo_l = (float)(g - (double)hi_l);
    }
#pragma unroll
    for (int k = 0; k < HF; ++k) {
        ghi[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hi_l), k));
        glo[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo_l), k));
    }
}

// two lanes per row (attn_rel_wide.hip, attn_rel_wide_shared.hip): x of this lane + x of its partner lane l ^ 32, as
// half0 + half1 on both
__device__ __forceinline__ float rel_pair_sum(float x) {
    const unsigned b = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);     // {x of lane l & 31, x of lane 32 + (l & 31)}
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}

// W contiguous floats at p (16-byte aligned), times mul
template <int W>
__device__ __forceinline__ void rel_load_row(float (&dst)[W], const float* __restrict__ p, float mul) {
#pragma unroll
    for (int d4 = 0; d4 < W / 4; ++d4) {
        const float4 v = *reinterpret_cast<const float4*>(p + 4 * d4);
        dst[4 * d4] = v.x * mul; dst[4 * d4 + 1] = v.y * mul; dst[4 * d4 + 2] = v.z * mul; dst[4 * d4 + 3] = v.w * mul;
    }
}

template <int W>
__device__ __forceinline__ void rel_store_row(float* __restrict__ p, const float (&src)[W], float mul) {
#pragma unroll
    for (int d4 = 0; d4 < W / 4; ++d4)
        *reinterpret_cast<float4*>(p + 4 * d4) =
            make_float4(src[4 * d4] * mul, src[4 * d4 + 1] * mul, src[4 * d4 + 2] * mul, src[4 * d4 + 3] * mul);
}

// the embedding half of a lane at head width 64, at p = row + head * 64 + 16 h: dst[k] = sine column p[k],
// dst[16 + k] = cosine column p[32 + k]
__device__ __forceinline__ void rel_load_emb(float (&dst)[32], const float* __restrict__ p, float mul) {
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int d4 = 0; d4 < 4; ++d4) {
            const float4 v = *reinterpret_cast<const float4*>(p + 32 * part + 4 * d4);
            float* d = dst + 16 * part + 4 * d4;
            d[0] = v.x * mul; d[1] = v.y * mul; d[2] = v.z * mul; d[3] = v.w * mul;
        }
}

__device__ __forceinline__ void rel_store_emb(float* __restrict__ p, const float (&src)[32], float mul) {
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int d4 = 0; d4 < 4; ++d4) {
            const float* s = src + 16 * part + 4 * d4;
            *reinterpret_cast<float4*>(p + 32 * part + 4 * d4) = make_float4(s[0] * mul, s[1] * mul, s[2] * mul, s[3] * mul);
        }
}

// the shared-embedding families: s_ij of a block row is [chunk j < W / 4][unit < UNITS][4 floats]; this unit's W values
template <int W, int UNITS>
__device__ __forceinline__ void rel_read(float (&sc)[W], const float* __restrict__ srow, int unit) {
#pragma unroll
    for (int j = 0; j < W / 4; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(srow + (j * UNITS + unit) * 4);
        sc[4 * j] = v.x; sc[4 * j + 1] = v.y; sc[4 * j + 2] = v.z; sc[4 * j + 3] = v.w;
    }
}

// Tile `tile` of the plan of gn_attention_plan -> its event's rows [kbeg, kend) and TILE0, the first row of the tile.  The one
// `return` (a tile past the plan's last) depends on `tile` alone: a workgroup leaves as a whole before its first barrier.
#define REL_EVENT_PROLOGUE(TILE0)                                                                               \
    if (tile >= tile_ptr[B]) return;                                                                            \
    const int es = rel_event_of_tile(tile_ptr, B, tile);                                                        \
    const int e = tile_ptr[B + 1 + es];                                                                         \
    const int kbeg = ptr[e], kend = ptr[e + 1];                                                                 \
    const int TILE0 = kbeg + (tile - tile_ptr[es]) * REL_TILE;

// Tile -> event and rows.  `lane` is the thread of the workgroup; ROWOFF (an expression of `lane`) is its row in the tile.
#define REL_TILE_PROLOGUE_AT(ROW0, ROWI, ROWOFF)                                                                \
    const int tile = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;                                         \
    REL_EVENT_PROLOGUE(ROW0)                                                                                    \
    const int E = H * DH;                                                                                       \
    const int ROWI = ROW0 + (ROWOFF);                                                                           \
    const bool valid = ROWI < kend;                                                                             \
    const int myrow = valid ? ROWI : kend - 1;

// ---- host side of every launcher ----
// Row pitches (in elements) of a forward (`bwd` false: lddo .. lddqp are not looked at) or a backward: multiples of `vec`
// elements = 16 bytes (4 fp32, 8 bf16) and at least the row width; xt holds x, y, z, time.
inline bool rel_args_ok(bool bwd, int vec, int H, int DH, long long ld, long long ldqp, long long ldxt, long long ldo,
                        long long ldu, long long lddo = 0, long long lddu = 0, long long lddq = 0, long long lddqp = 0) {
    const long long d = (long long)H * DH;
    if (ld % vec || ldqp % vec || ldo % vec || ldu % vec || ldxt < 4 || ld < 3 * d || ldqp < d || ldo < d || ldu < d) return false;
    return !bwd || !(lddo % vec || lddu % vec || lddq % vec || lddqp % vec || lddq < 3 * d || lddo < d || lddu < d || lddqp < d);
}

// more than 64 KB of dynamic LDS has to be asked for once per kernel
template <typename K>
inline hipError_t rel_allow_lds(K kernel, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// what the scores are scaled by: 1 / sqrt(dh), and the same in the exp2 domain
inline float rel_scale(int DH) { return 1.0f / sqrtf((float)DH); }
inline float rel_scale2(int DH) { return REL_LOG2E / sqrtf((float)DH); }

}  // namespace gn
