// graphnet_amd/csrc/row_math.hpp — the activation and wave-reduction helpers of the row kernels (generic.hip), shared with the
// fused LayerNorm + GELU edge kernels (edgeconv_norm.hip) so that both families evaluate the same expressions.
#pragma once
#include "common.hpp"

namespace gn {

// ---------------------------------------------------------------- activations
// ACT: 0 = relu, 1 = gelu (erf form, torch.nn.GELU() default), 2 = leaky relu (slope 0.01, torch default),
//      3 = identity
// Phi(y) = 0.5 (1 + erf(y / sqrt 2)) and e = exp(-y^2 / 2) for GELU and its derivative.  erf by Abramowitz & Stegun 7.1.26
// (|error| <= 1.5e-7: below fp32 rounding of Phi): one v_rcp_f32, one v_exp_f32 and six FMAs, where the library's erff + expf
// were ~70 vector instructions per element - the GELU row kernels were bound by exactly that (6 elements per lane and row).
__device__ __forceinline__ float gelu_phi(float y, float* e_out) {
    const float x = __builtin_fabsf(y) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, x, 1.0f));
    const float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * x * x);                 // exp(-x^2) = exp(-y^2 / 2)
    float p = 1.061405429f;
    p = __builtin_fmaf(p, t, -1.453152027f);
    p = __builtin_fmaf(p, t, 1.421413741f);
    p = __builtin_fmaf(p, t, -0.284496736f);
    p = __builtin_fmaf(p, t, 0.254829592f);
    const float erf_abs = __builtin_fmaf(-p * t, e, 1.0f);                                // erf(|y| / sqrt 2)
    *e_out = e;
    return __builtin_fmaf(0.5f, __builtin_copysignf(erf_abs, y), 0.5f);
}
template <int ACT> __device__ __forceinline__ float act_fwd(float y) {
    if constexpr (ACT == 0) return fmaxf(y, 0.0f);
    else if constexpr (ACT == 1) { float e; return y * gelu_phi(y, &e); }
    else if constexpr (ACT == 2) return y > 0.0f ? y : 0.01f * y;
    else return y;
}
template <int ACT> __device__ __forceinline__ float act_grad(float y) {
    if constexpr (ACT == 0) return y > 0.0f ? 1.0f : 0.0f;
    else if constexpr (ACT == 1) { float e; const float phi = gelu_phi(y, &e); return __builtin_fmaf(y * 0.39894228040143267794f, e, phi); }
    else if constexpr (ACT == 2) return y > 0.0f ? 1.0f : 0.01f;
    else return 1.0f;
}

// Wave-wide sum, every lane gets it: the xor butterfly 32, 16, 8, 4, 2, 1 - bit for bit what the __shfl_xor loop returns
// (tools/probe/wave_sum_probe.hip) - without the LDS crossbar: the row kernels do two to four of these per ROW and
// ds_bpermute (6 per sum) was what bound them.  v_permlane32_swap / v_permlane16_swap (gfx950) exchange the wave's halves /
// the rows' neighbours, DPP row_ror:8, row_shl:4 | row_shr:4 and two quad_perms do the rest on the vector ALU.
__device__ __forceinline__ float wave_sum(float v) {
    const int lane = threadIdx.x & 63;
    {
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        v += __builtin_bit_cast(float, lane < 32 ? r[1] : r[0]);
    }
    {
        const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v), __builtin_bit_cast(unsigned, v), false, false);
        v += __builtin_bit_cast(float, (lane & 16) ? r[0] : r[1]);
    }
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
    {
        const int up = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x104, 0xf, 0xf, false);             // row_shl:4
        const int dn = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, false);             // row_shr:4
        v += __builtin_bit_cast(float, (lane & 4) ? dn : up);
    }
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    return v;
}

}  // namespace gn
