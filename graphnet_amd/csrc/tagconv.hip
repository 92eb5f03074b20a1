// graphnet_amd/csrc/tagconv.hip — TAGConv(K = 2) of ConvNet: propagation with the symmetrically normalised adjacency.
//
//   dis[i]   = deg[i] > 0 ? deg[i]^-1/2 : 0          deg = valid entries of table row i, overflow entry included
//   (P x)_i  = dis[i] * sum_{j -> i} dis[j] * x_j     slots 0..K-1 in order, then the overflow entry
//   out      = leaky_relu(x W0^T + (P x) W1^T + (P P x) W2^T + b, 0.01)
//
// Kernels (fp32 rows in HBM in both compute modes, no atomics, every sum in a fixed order):
//   tag_norm_kernel         dis from the table
//   tag_propagate_kernel    h = P x: a gather.  A centre is served by C/4 lanes (one 16-byte load per lane and neighbour), so a wave
//                           holds 64 / (C/4) centres; the slot loop runs four neighbour rows at a time
//   tag_propagate_t_kernel  out = add + P^T g over the reverse lists (one wave per node; lists of <= 64 rows are ordered in the wave,
//                           as dq_gather_kernel of edgeconv.hip does), tag_hub_t_kernel: 16 waves per hub node
//   tagconv_fwd_kernel<T>   one layer: a workgroup owns 32 centres.  It stages [x | h1 | h2] of the tile as the LDS A operand
//                           ([32][3C] of T, rows padded by 16 bytes), gathering h2 = P h1 on the way in (h2 also goes to HBM once for the
//                           weight gradient), then wave w multiplies the tile with the 32-column blocks w and w + 4 of [W0 | W1 | W2]^T.
//                           The weight fragments come straight from global memory (each lane reads 16 consecutive bytes of one weight
//                           row per k-step; the 3C x Cout matrix stays in L2), bias and leaky ReLU are applied on the accumulators.
//   tag_dpre_kernel         dpre = dout * (out > 0 ? 1 : 0.01)
#include "launchers.hpp"

namespace gn {
namespace {

constexpr int TAG_TM = 32;                       // centres per tile of the fused layer
constexpr float TAG_SLOPE = 0.01f;
constexpr int TAG_HUB_MIN = 64, TAG_HUB_CAP = 16384;     // = REV_SORT_MIN / REV_SORT_CAP of graph.hip
constexpr int TAG_HUB_WAVES = 16;

__device__ __forceinline__ void fma4(float w, const float4& v, float4& a) {
    a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
}

__global__ __launch_bounds__(256) void tag_norm_kernel(const int* __restrict__ nbr, const int* __restrict__ ovf, int N, int K,
                                                       float* __restrict__ dis) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int deg = (ovf && ovf[i] >= 0) ? 1 : 0;
    for (int s = 0; s < K; ++s) deg += nbr[(long long)i * K + s] >= 0 ? 1 : 0;
    dis[i] = deg > 0 ? 1.0f / sqrtf((float)deg) : 0.0f;
}

// columns [col, col + 4) of (P x)_i
__device__ __forceinline__ float4 tag_gather(const float* __restrict__ x, long long ldx, const float* __restrict__ dis,
                                             const int* __restrict__ nbr, const int* __restrict__ ovf, int i, int K, int col) {
    const int* row = nbr + (long long)i * K;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 4 <= K; s += 4) {
        float w[4];
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = row[s + u];
            w[u] = 0.f;
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 0) {
                w[u] = dis[j];
                v[u] = *reinterpret_cast<const float4*>(x + (long long)j * ldx + col);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) fma4(w[u], v[u], acc);       // an empty slot adds 0 * 0: exact
    }
    for (; s <= K; ++s) {                                        // the tail slots, then the overflow entry (s == K)
        if (s == K && !ovf) break;
        const int j = s < K ? row[s] : ovf[i];
        if (j >= 0) fma4(dis[j], *reinterpret_cast<const float4*>(x + (long long)j * ldx + col), acc);
    }
    const float di = dis[i];
    return make_float4(di * acc.x, di * acc.y, di * acc.z, di * acc.w);
}

__global__ __launch_bounds__(256) void tag_propagate_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ dis,
                                                            const int* __restrict__ nbr, const int* __restrict__ ovf, int N, int K,
                                                            int C, float* __restrict__ h, long long ldh) {
    const int lpc = C >> 2, cpw = 64 / lpc;                      // lanes per centre, centres per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / lpc, l = lane - grp * lpc;
    const long long i = ((long long)blockIdx.x * 4 + wave) * cpw + grp;
    if (grp >= cpw || i >= N) return;
    const float4 a = tag_gather(x, ldx, dis, nbr, ovf, (int)i, K, l * 4);
    *reinterpret_cast<float4*>(h + i * ldh + l * 4) = a;
}

// centre of edge row r (row = i*S + slot, or N*S + t for overflow row t)
__device__ __forceinline__ int tag_row_centre(int r, int NS, int S, const int* __restrict__ ovf_centre) {
    return r < NS ? r / S : ovf_centre[r - NS];
}

__global__ __launch_bounds__(256) void tag_propagate_t_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ add,
                                                              long long lda, const float* __restrict__ dis,
                                                              const int* __restrict__ rev_ptr, const int* __restrict__ rev_rows,
                                                              const int* __restrict__ ovf_centre, int N, int S, int C,
                                                              float* __restrict__ out, long long ldo) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= N) return;
    const int lo = rev_ptr[j], hi = rev_ptr[j + 1];
    const int deg = hi - lo, NS = N * S;
    if (deg > TAG_HUB_MIN && deg <= TAG_HUB_CAP) return;         // tag_hub_t_kernel sums this node
    const int col = lane * 4;
    const bool ok = col < C;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (deg <= 64) {
        // the list is in the order its atomics came in: rank the row ids in the wave, walk them in ascending order
        const int r = lane < deg ? rev_rows[lo + lane] : 0x7fffffff;
        int rank = 0;
        for (int t = 0; t < deg; ++t) rank += (__shfl(r, t) < r) ? 1 : 0;      // row ids are distinct
        const int sorted = __builtin_amdgcn_ds_permute((lane < deg ? rank : lane) << 2, r);
        const int c = lane < deg ? tag_row_centre(sorted, NS, S, ovf_centre) : 0;
        const float w = lane < deg ? dis[c] : 0.f;
        for (int t = 0; t < deg; t += 8) {
            float wu[8];
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = min(t + u, deg - 1);
                const int cu = __shfl(c, e);
                wu[u] = t + u < deg ? __shfl(w, e) : 0.f;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok && t + u < deg) v[u] = *reinterpret_cast<const float4*>(g + (long long)cu * ldg + col);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) fma4(wu[u], v[u], acc);
        }
    } else {
        // beyond the sort capacity: next row id in ascending order = min over the entries above the last one
        int last = -1;
        for (int t = lo; t < hi; ++t) {
            int best = 0x7fffffff;
            for (int e = lo + lane; e < hi; e += 64) {
                const int r = rev_rows[e];
                if (r > last && r < best) best = r;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
            last = best;
            const int c = tag_row_centre(best, NS, S, ovf_centre);
            if (ok) fma4(dis[c], *reinterpret_cast<const float4*>(g + (long long)c * ldg + col), acc);
        }
    }
    if (ok) {
        const float dj = dis[j];
        float4 a = add ? *reinterpret_cast<const float4*>(add + (long long)j * lda + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        a.x = fmaf(dj, acc.x, a.x); a.y = fmaf(dj, acc.y, a.y); a.z = fmaf(dj, acc.z, a.z); a.w = fmaf(dj, acc.w, a.w);
        *reinterpret_cast<float4*>(out + (long long)j * ldo + col) = a;
    }
}

// Hub nodes (sorted reverse lists of 65..16384 rows): one 16-wave workgroup per hub.  Wave w sums the row blocks w, w + 16, ...
// (8 rows each, loaded together) in ascending order; the 16 partial sums are added in wave order.
__global__ __launch_bounds__(TAG_HUB_WAVES * 64) void tag_hub_t_kernel(const float* __restrict__ g, long long ldg,
                                                                       const float* __restrict__ add, long long lda,
                                                                       const float* __restrict__ dis, const int* __restrict__ rev_ptr,
                                                                       const int* __restrict__ rev_rows,
                                                                       const int* __restrict__ ovf_centre,
                                                                       const int* __restrict__ hubs, const int* __restrict__ nhubs,
                                                                       int N, int S, int C, float* __restrict__ out, long long ldo) {
    __shared__ float part[TAG_HUB_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane * 4, NS = N * S;
    const bool ok = col < C;
    const int n = *nhubs;
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        const int j = hubs[t];
        const int lo = rev_ptr[j], deg = rev_ptr[j + 1] - lo;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b0 = wave * 8; b0 < deg; b0 += TAG_HUB_WAVES * 8) {
            float wu[8];
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                wu[u] = 0.f;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b0 + u < deg) {
                    const int c = tag_row_centre(rev_rows[lo + b0 + u], NS, S, ovf_centre);
                    wu[u] = dis[c];
                    if (ok) v[u] = *reinterpret_cast<const float4*>(g + (long long)c * ldg + col);
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) fma4(wu[u], v[u], acc);
        }
        if (ok) *reinterpret_cast<float4*>(&part[wave][col]) = acc;
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += TAG_HUB_WAVES * 64) {
            float s = part[0][c];
#pragma unroll
            for (int w = 1; w < TAG_HUB_WAVES; ++w) s += part[w][c];
            const float a = add ? add[(long long)j * lda + c] : 0.f;
            out[(long long)j * ldo + c] = fmaf(dis[j], s, a);
        }
        __syncthreads();
    }
}

template <typename T> __device__ __forceinline__ Frag<T> frag_at(const unsigned char* p) {
    Frag<T> f;
    if constexpr (sizeof(T) == 4) f.v = *reinterpret_cast<const f32x4*>(p);
    else f.v = *reinterpret_cast<const bf16x8*>(p);
    return f;
}

template <typename T>
__global__ __launch_bounds__(256) void tagconv_fwd_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ h1,
                                                          long long ldh1, const float* __restrict__ dis, const int* __restrict__ nbr,
                                                          const int* __restrict__ ovf, int N, int K, int C,
                                                          const T* __restrict__ Wp, const float* __restrict__ bias, int Cout,
                                                          float* __restrict__ h2, long long ldh2, float* __restrict__ out,
                                                          long long ldo) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tag_a[];      // [TAG_TM][3C] of T, row pitch 3C*sizeof(T) + 16
    const int K3 = 3 * C;
    const int pitch = K3 * (int)sizeof(T) + 16;
    const int lpc = C >> 2, cpw = 64 / lpc;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i0 = (long long)blockIdx.x * TAG_TM;

    // segments 0 and 1: the tile's own x and h1 rows (rows past N: zeros)
    for (int idx = threadIdx.x; idx < TAG_TM * 2 * lpc; idx += 256) {
        const int row = idx / (2 * lpc), rem = idx - row * 2 * lpc;
        const int seg = rem / lpc, l = rem - seg * lpc;
        const long long i = i0 + row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < N) v = *reinterpret_cast<const float4*>(seg ? h1 + i * ldh1 + l * 4 : x + i * ldx + l * 4);
        store4<T>(tag_a + row * pitch + (seg * C + l * 4) * (int)sizeof(T), v.x, v.y, v.z, v.w);
    }
    // segment 2: h2 = P h1, wave w gathers the rows 8w .. 8w + 7, cpw of them at a time
    {
        const int grp = lane / lpc, l = lane - grp * lpc;
        for (int r0 = 0; r0 < TAG_TM / 4; r0 += cpw) {
            if (grp >= cpw) break;
            const int row = wave * (TAG_TM / 4) + r0 + grp;
            const long long i = i0 + row;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < N) {
                v = tag_gather(h1, ldh1, dis, nbr, ovf, (int)i, K, l * 4);
                *reinterpret_cast<float4*>(h2 + i * ldh2 + l * 4) = v;
            }
            store4<T>(tag_a + row * pitch + (2 * C + l * 4) * (int)sizeof(T), v.x, v.y, v.z, v.w);
        }
    }
    __syncthreads();

    const int NT = Cout >> 5;
    if (wave >= NT) return;
    const bool two = wave + 4 < NT;
    const int r = lane & 31, hh = lane >> 5;
    const unsigned char* ap = tag_a + r * pitch + hh * 16;
    const unsigned char* bp0 = reinterpret_cast<const unsigned char*>(Wp) + (long long)(wave * 32 + r) * K3 * (int)sizeof(T) + hh * 16;
    const unsigned char* bp1 = bp0 + (long long)128 * K3 * (int)sizeof(T);
    f32x16 acc0, acc1;
    zero_acc(acc0);
    zero_acc(acc1);
    constexpr int U = 6;                                          // 3C*sizeof(T)/32 k-steps: a multiple of 6 (bf16) or 12 (fp32)
    const int nsteps = K3 * (int)sizeof(T) / 32;
    for (int s = 0; s < nsteps; s += U) {
        Frag<T> fa[U], fb0[U], fb1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) fb0[u] = frag_at<T>(bp0 + (s + u) * 32);
        if (two) {
#pragma unroll
            for (int u = 0; u < U; ++u) fb1[u] = frag_at<T>(bp1 + (s + u) * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) fa[u] = frag_at<T>(ap + (s + u) * 32);
#pragma unroll
        for (int u = 0; u < U; ++u) mma(fa[u], fb0[u], acc0);
        if (two) {
#pragma unroll
            for (int u = 0; u < U; ++u) mma(fa[u], fb1[u], acc1);
        }
    }
    // epilogue: bias + leaky ReLU on the accumulators (col = lane & 31, row = acc_row(reg, lane >> 5))
    const int col0 = wave * 32 + r;
    const float b0 = bias ? bias[col0] : 0.f;
    const float b1 = (bias && two) ? bias[col0 + 128] : 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const long long i = i0 + acc_row(q, hh);
        if (i < N) {
            float v = acc0[q] + b0;
            out[i * ldo + col0] = v > 0.f ? v : TAG_SLOPE * v;
            if (two) {
                v = acc1[q] + b1;
                out[i * ldo + col0 + 128] = v > 0.f ? v : TAG_SLOPE * v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void tag_dpre_kernel(const float* __restrict__ dout, long long lddo, const float* __restrict__ out,
                                                       long long ldo, long long N, int C, float* __restrict__ dpre, long long ldp) {
    const int c4 = C >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * c4) return;
    const long long i = idx / c4;
    const int col = (int)(idx - i * c4) * 4;
    const float4 d = *reinterpret_cast<const float4*>(dout + i * lddo + col);
    const float4 o = *reinterpret_cast<const float4*>(out + i * ldo + col);
    *reinterpret_cast<float4*>(dpre + i * ldp + col) =
        make_float4(o.x > 0.f ? d.x : TAG_SLOPE * d.x, o.y > 0.f ? d.y : TAG_SLOPE * d.y, o.z > 0.f ? d.z : TAG_SLOPE * d.z,
                    o.w > 0.f ? d.w : TAG_SLOPE * d.w);
}

inline bool tag_width_ok(int C) { return C >= 32 && C <= 256 && C % 32 == 0; }
inline bool tag_row_ok(const void* p, long long ld, int C) { return p && ld >= C && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int cdiv_(long long a, long long b) { return (int)((a + b - 1) / b); }

}  // namespace

bool tagconv_supported(int C_in, int C_out) { return tag_width_ok(C_in) && tag_width_ok(C_out); }

hipError_t launch_tag_norm(const int* nbr, const int* ovf, int N, int K, float* dis, hipStream_t st) {
    if (N < 0 || K < 1 || K > 32 || (N > 0 && (!nbr || !dis))) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(tag_norm_kernel, dim3(cdiv_(N, 256)), dim3(256), 0, st, nbr, ovf, N, K, dis);
    return hipGetLastError();
}

hipError_t launch_tag_propagate(const float* x, long long ldx, const float* dis, const int* nbr, const int* ovf, int N, int K, int C,
                                float* h, long long ldh, hipStream_t st) {
    if (N < 0 || K < 1 || K > 32 || !tag_width_ok(C)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    if (!tag_row_ok(x, ldx, C) || !tag_row_ok(h, ldh, C) || !dis || !nbr) return hipErrorInvalidValue;
    const int cpw = 64 / (C / 4);
    hipLaunchKernelGGL(tag_propagate_kernel, dim3(cdiv_(N, 4 * cpw)), dim3(256), 0, st, x, ldx, dis, nbr, ovf, N, K, C, h, ldh);
    return hipGetLastError();
}

hipError_t launch_tag_propagate_t(const float* g, long long ldg, const float* add, long long lda, const float* dis,
                                  const int* rev_ptr, const int* rev_rows, const int* hubs, const int* nhubs, const int* ovf_centre,
                                  int N, int K, int C, float* out, long long ldo, hipStream_t st) {
    if (N < 0 || K < 1 || K > 32 || !tag_width_ok(C)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    if (!tag_row_ok(g, ldg, C) || !tag_row_ok(out, ldo, C) || (add && !tag_row_ok(add, lda, C)) || !dis || !rev_ptr || !rev_rows ||
        !hubs || !nhubs)
        return hipErrorInvalidValue;
    const int S = edge_slots(K);
    if ((long long)N * S + N > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tag_propagate_t_kernel, dim3(cdiv_(N, 4)), dim3(256), 0, st, g, ldg, add, lda, dis, rev_ptr, rev_rows,
                       ovf_centre, N, S, C, out, ldo);
    hipLaunchKernelGGL(tag_hub_t_kernel, dim3(256), dim3(TAG_HUB_WAVES * 64), 0, st, g, ldg, add, lda, dis, rev_ptr, rev_rows,
                       ovf_centre, hubs, nhubs, N, S, C, out, ldo);
    return hipGetLastError();
}

hipError_t launch_tagconv_fwd(int mode, const float* x, long long ldx, const float* h1, long long ldh1, const float* dis,
                              const int* nbr, const int* ovf, int N, int K, int C_in, const void* Wp, const float* bias, int C_out,
                              float* h2, long long ldh2, float* out, long long ldo, hipStream_t st) {
    if ((mode != 0 && mode != 1) || N < 0 || K < 1 || K > 32 || !tagconv_supported(C_in, C_out)) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    if (!tag_row_ok(x, ldx, C_in) || !tag_row_ok(h1, ldh1, C_in) || !tag_row_ok(h2, ldh2, C_in) || !tag_row_ok(out, ldo, C_out) ||
        !dis || !nbr || !Wp || (reinterpret_cast<uintptr_t>(Wp) & 15))
        return hipErrorInvalidValue;
    const dim3 grid(cdiv_(N, TAG_TM)), block(256);
    if (mode == 0) {
        const int lds = TAG_TM * (3 * C_in * 4 + 16);
        static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(&tagconv_fwd_kernel<float>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, TAG_TM * (3 * 256 * 4 + 16));
        if (once != hipSuccess) return once;
        hipLaunchKernelGGL((tagconv_fwd_kernel<float>), grid, block, lds, st, x, ldx, h1, ldh1, dis, nbr, ovf, N, K, C_in,
                           (const float*)Wp, bias, C_out, h2, ldh2, out, ldo);
    } else {
        const int lds = TAG_TM * (3 * C_in * 2 + 16);
        hipLaunchKernelGGL((tagconv_fwd_kernel<__bf16>), grid, block, lds, st, x, ldx, h1, ldh1, dis, nbr, ovf, N, K, C_in,
                           (const __bf16*)Wp, bias, C_out, h2, ldh2, out, ldo);
    }
    return hipGetLastError();
}

hipError_t launch_tag_dpre(const float* dout, long long lddo, const float* out, long long ldo, long long N, int C, float* dpre,
                           long long ldp, hipStream_t st) {
    if (N < 0 || C < 4 || C % 4) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    if (!tag_row_ok(dout, lddo, C) || !tag_row_ok(out, ldo, C) || !tag_row_ok(dpre, ldp, C)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tag_dpre_kernel, dim3(cdiv_(N * (C / 4), 256)), dim3(256), 0, st, dout, lddo, out, ldo, N, C, dpre, ldp);
    return hipGetLastError();
}

}  // namespace gn
