// graphnet_amd/csrc/attn_rel.hpp — what the two kernel families of the spacetime-bias attention share (attn_rel.hip: head
// width 32, one lane per query; attn_rel_wide.hip: head width 64, two lanes per query): the tile prologue over the plan of
// gn_attention_plan, the LDS staging, and the pair argument with its sine / cosine (a CONTRACT, include/graphnet_amd.h).
#pragma once
#include "common.hpp"

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

// Tile -> event and rows.  `lane` is the thread of the workgroup; ROWOFF (an expression of `lane`) is its row in the tile.
#define REL_TILE_PROLOGUE_AT(ROW0, ROWI, ROWOFF)                                                                \
    const int tile = blockIdx.x, head = blockIdx.y, lane = threadIdx.x;                                         \
    if (tile >= tile_ptr[B]) return;                                                                            \
    const int es = rel_event_of_tile(tile_ptr, B, tile);                                                        \
    const int e = tile_ptr[B + 1 + es];                                                                         \
    const int kbeg = ptr[e], kend = ptr[e + 1];                                                                 \
    const int ROW0 = kbeg + (tile - tile_ptr[es]) * REL_TILE;                                                   \
    const int E = H * DH;                                                                                       \
    const int ROWI = ROW0 + (ROWOFF);                                                                           \
    const bool valid = ROWI < kend;                                                                             \
    const int myrow = valid ? ROWI : kend - 1;

}  // namespace gn
