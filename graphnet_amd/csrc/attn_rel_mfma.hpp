// graphnet_amd/csrc/attn_rel_mfma.hpp — what the two matrix-core families of the spacetime-bias attention share
// (attn_rel_mfma.hip: head width 32; attn_rel_mfma_wide.hip: 64): the bf16 product wrappers, the one rounding to bf16
// (rm_pack4), the transposed LDS operand read and the delta kernel of the backward.
#pragma once
#include "attn_rel.hpp"

namespace gn {

typedef short rm_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) rm_s16x4 rm_lds_s16x4;

__device__ __forceinline__ float rm_exp2(float x) { return __builtin_amdgcn_exp2f(x); }       // bare v_exp_f32: exp2(-inf) = 0
__device__ __forceinline__ f32x4 rm_mma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 rm_mma16(rm_s16x4 a, rm_s16x4 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void rm_zero(f32x4& a) { a = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }       // (common.hpp's zero_acc is for 16 registers)
__device__ __forceinline__ bf16x8 rm_ld8(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ rm_s16x4 rm_pack4(float a, float b, float c, float d) {
    bf16x4 v;
    v[0] = (__bf16)a; v[1] = (__bf16)b; v[2] = (__bf16)c; v[3] = (__bf16)d;
    return __builtin_bit_cast(rm_s16x4, v);
}
__device__ __forceinline__ void rm_store4(__bf16* p, float a, float b, float c, float d) {
    *reinterpret_cast<rm_s16x4*>(p) = rm_pack4(a, b, c, d);
}
// 16x16x16 operand (A: row = l & 15, B: column = l & 15; k = 4 (l >> 4) .. + 3) TRANSPOSED out of a row-major bf16 tile: element
// (k, col0 + (l & 15)) of the tile at `tile` with `pitch` elements per row.  The 16 lanes of a group address the 4 rows x 16 columns
// they share, lane (l & 15) the 4 columns 4 (l & 3) .. of row (l & 15) >> 2, and each receives the 4 rows of its own column.
__device__ __forceinline__ rm_s16x4 rm_tr(const __bf16* tile, int pitch, int col0, int lane) {
    const int li = lane & 15, g4 = lane >> 4;
    const __bf16* p = tile + (4 * g4 + (li >> 2)) * pitch + col0 + 4 * (li & 3);
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((rm_lds_s16x4*)(p));
}

// delta[i, h] = dU_i . U_i + dO_i . O_i (fp32, one thread per (row, head)) for both backward passes
template <int DH>
__global__ __launch_bounds__(256) void rel_attn_mfma_delta_kernel(
    const __bf16* __restrict__ out, long long ldo, const __bf16* __restrict__ u, long long ldu, const __bf16* __restrict__ dout,
    long long lddo, const __bf16* __restrict__ du, long long lddu, int H, long long NH, float* __restrict__ delta) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= NH) return;
    const long long row = idx / H;
    const int col = (int)(idx % H) * DH;
    float dl = 0.0f;
#pragma unroll
    for (int c8 = 0; c8 < DH / 8; ++c8) {
        const bf16x8 a = rm_ld8(du + row * lddu + col + 8 * c8), b = rm_ld8(u + row * ldu + col + 8 * c8);
#pragma unroll
        for (int i = 0; i < 8; ++i) dl = fmaf((float)a[i], (float)b[i], dl);
    }
#pragma unroll
    for (int c8 = 0; c8 < DH / 8; ++c8) {
        const bf16x8 a = rm_ld8(dout + row * lddo + col + 8 * c8), b = rm_ld8(out + row * ldo + col + 8 * c8);
#pragma unroll
        for (int i = 0; i < 8; ++i) dl = fmaf((float)a[i], (float)b[i], dl);
    }
    delta[idx] = dl;
}

}  // namespace gn
