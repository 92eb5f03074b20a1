// graphnet_amd/csrc/generic.hip — unfused building blocks for the DynEdge variants the fused kernels do
// not cover: activation_layer="gelu" and add_norm_layer=True (LayerNorm after every Linear of the edge and
// post-processing MLPs; models/gnn/dynedge.py:160-167,198-231).
//
// With GELU or LayerNorm the backward needs the pre-activations themselves (not one relu bit), and LayerNorm
// reduces over a whole edge row, so these variants run the edge MLP unfused, on edge-row tensors in HBM:
//     pre1[r] = P[i_r] + Q[j_r]            edge_gather_pre      (same algebraic split as the fused path)
//     a1 = act(LN(pre1))                   rownorm_act_fwd
//     z2 = a1 . W2^T + b2                  gemm (gemm.hip), M = edge rows
//     m  = act(LN(z2)), 0 on empty slots   rownorm_act_fwd
//     out[i] = sum_slots m                 slot_sum
// and the mirror image backwards (rownorm_act_bwd, the same GEMM / wgrad kernels, slot_sum for dP, the
// reverse-adjacency gather for dQ).  All HBM-bound elementwise / row-reduction kernels: one wave per row.
#include "common.hpp"
#include "row_math.hpp"

namespace gn {

// ---------------------------------------------------------------- edge row -> (centre, source)
__global__ __launch_bounds__(256) void edge_rows_kernel(EdgeGraph g, int S, int* __restrict__ ic, int* __restrict__ jc,
                                                        long long rows) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows) return;
    const long long main_rows = (long long)g.N * S;
    int i = 0, j = -1;
    if (t < main_rows) {
        i = (int)(t / S);
        const int s = (int)(t % S);
        if (s < g.K) j = g.nbr[(long long)i * g.K + s];
    } else if (g.ovf_cnt && t - main_rows < *g.ovf_cnt) {
        i = g.ovf_centre[t - main_rows];
        j = g.ovf_src[t - main_rows];
    }
    ic[t] = i;
    jc[t] = j;
}

// element of an fp32 or (lowp) bf16 tensor
__device__ __forceinline__ float ld_f32_or_bf16(const float* p, long long i, bool lowp) {
    return lowp ? (float)reinterpret_cast<const __bf16*>(p)[i] : p[i];
}
// ---------------------------------------------------------------- compact edge rows (existing edges only)
// The S-slot row layout above has 16 slots per centre for k = 9 (DeepIce's embedded DynEdge): 17 N rows of which 9 N exist.
// Compact rows: row_ptr[i] .. row_ptr[i + 1] are centre i's edges - its table slots in slot order, then its overflow edge -
// so every row kernel and GEMM of the unfused path runs on the existing edges only.
// deg[i] = edges of centre i (the scan of it is row_ptr)
__global__ __launch_bounds__(256) void rows_degree_kernel(EdgeGraph g, const int* __restrict__ ovf, int* __restrict__ deg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.N) return;
    int d = 0;
    for (int s = 0; s < g.K; ++s) d += g.nbr[(long long)i * g.K + s] >= 0 ? 1 : 0;
    if (ovf && ovf[i] >= 0) ++d;
    deg[i] = d;
}
// ic / jc beyond row_ptr[N] stay (0, -1) (filled by the launcher)
__global__ __launch_bounds__(256) void rows_compact_fill_kernel(EdgeGraph g, const int* __restrict__ ovf, const int* __restrict__ row_ptr,
                                                                int* __restrict__ ic, int* __restrict__ jc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.N) return;
    int at = row_ptr[i];
    for (int s = 0; s < g.K; ++s) {
        const int j = g.nbr[(long long)i * g.K + s];
        if (j >= 0) { ic[at] = i; jc[at] = j; ++at; }
    }
    if (ovf && ovf[i] >= 0) { ic[at] = i; jc[at] = ovf[i]; }
}
// out[i, c] = sum of m[r, c] over centre i's rows, in row order (= slot order, overflow edge last: the order and the terms of
// slot_sum_kernel + slot_sum_ovf_kernel, whose other terms are zeros)
__global__ __launch_bounds__(256) void segment_rows_sum_kernel(const float* __restrict__ m, long long ldm, int C, int N,
                                                               const int* __restrict__ row_ptr, float* __restrict__ out, long long ldo,
                                                               int m_lowp) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / C), c = (int)(t % C);
    if (i >= N) return;
    float s = 0.0f;
    for (int r = row_ptr[i]; r < row_ptr[i + 1]; ++r) s += ld_f32_or_bf16(m, (long long)r * ldm + c, m_lowp != 0);
    out[(long long)i * ldo + c] = s;
}
// reverse lists in compact row ids: S-layout row i * S + s -> row_ptr[i] + (existing slots before s); overflow row
// N * S + t -> the last row of its centre
__global__ __launch_bounds__(256) void rev_rows_compact_kernel(EdgeGraph g, int S, const int* __restrict__ row_ptr,
                                                               const int* __restrict__ rev_ptr, const int* __restrict__ rev_rows,
                                                               int* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rev_ptr[g.N]) return;
    const long long r = rev_rows[e];
    const long long main_rows = (long long)g.N * S;
    if (r < main_rows) {
        const int i = (int)(r / S), s = (int)(r % S);
        int rank = 0;
        for (int u = 0; u < s; ++u) rank += g.nbr[(long long)i * g.K + u] >= 0 ? 1 : 0;
        out[e] = row_ptr[i] + rank;
    } else {
        out[e] = row_ptr[g.ovf_centre[r - main_rows] + 1] - 1;
    }
}

// (activations act_fwd / act_grad and the wave-wide sum wave_sum: row_math.hpp)
// pre[r, 0:H1p] = act(P[ic[r]] + Q[jc[r]])  (PQ fp32 [N, 2*H1p]); rows without an edge -> 0.  ACT = identity
// gives the pre-activation (GELU / LayerNorm variants need it); a sign-preserving activation (leaky relu) can be
// applied here directly - its derivative is recovered from the sign of the result, nothing else is stored.
template <int ACT, typename OutT>
__global__ __launch_bounds__(256) void edge_gather_pre_kernel(const float* __restrict__ PQ, int H1p,
                                                              const int* __restrict__ ic, const int* __restrict__ jc,
                                                              long long rows, OutT* __restrict__ pre) {
    const int q4 = H1p >> 2;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = t / q4;
    const int c = (int)(t % q4) * 4;
    if (r >= rows) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int j = jc[r];
    if (j >= 0) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(PQ + (long long)ic[r] * 2 * H1p + c);
        const f32x4 q = *reinterpret_cast<const f32x4*>(PQ + (long long)j * 2 * H1p + H1p + c);
        v = p + q;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = act_fwd<ACT>(v[e]);
    }
    store4<OutT>(pre + r * H1p + c, v[0], v[1], v[2], v[3]);
}

constexpr int RN_MAXC = 512;             // columns per row handled by one wave (8 per lane)
constexpr int RN_PER = RN_MAXC / 64;

// a[r, c] = act(NORM ? LN(z[r, 0:C]) : z[r, c]) for c < C, 0 for C <= c < Cpad and for rows with valid[r] < 0.
// stats[r] = (mean, rstd) when NORM.  One wave per row.  (Measured at 2.7 TB/s of reads + writes on [1.5e6, 352] bf16 rows and
// not moved by any of: four rows per wave with all loads issued first, 16 / 8-byte accesses per lane, a cheaper erf, wave
// sums off the LDS crossbar - DESIGN.md 7h.)
template <bool NORM, int ACT, int NK>        // NK = columns per lane = ceil(Cpad / 64): the loops stop there
__global__ __launch_bounds__(256) void rownorm_act_fwd_kernel(
    const float* __restrict__ z, long long ldz, int C, const int* __restrict__ valid,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    float* __restrict__ a, long long lda, int Cpad, float* __restrict__ stats, long long rows,
    __bf16* __restrict__ a16, long long lda16,          // a and / or a16 (bf16 copy for the GEMMs that consume it)
    int z_lowp)                                         // z holds bf16 values (ldz in elements)
{
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const bool ok = !valid || valid[r] >= 0;
    float v[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        v[k] = (ok && c < C) ? ld_f32_or_bf16(z, r * ldz + c, z_lowp != 0) : 0.0f;
    }
    float mean = 0.0f, rstd = 1.0f;
    if constexpr (NORM) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; ++k) s += v[k];
        mean = wave_sum(s) / (float)C;
        float q = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            const float d = c < C ? v[k] - mean : 0.0f;
            q += d * d;
        }
        rstd = rsqrtf(wave_sum(q) / (float)C + eps);
        if (lane == 0 && stats) { stats[2 * r] = mean; stats[2 * r + 1] = rstd; }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = lane + 64 * k;
        if (c < Cpad) {
            float o = 0.0f;
            if (ok && c < C) {
                float y = v[k];
                if constexpr (NORM) y = (y - mean) * rstd * gamma[c] + beta[c];
                o = act_fwd<ACT>(y);
            }
            if (a) a[r * lda + c] = o;
            if (a16) a16[r * lda16 + c] = (__bf16)o;
        }
    }
}

// Backward of the above.  g: upstream gradient of a, row gidx ? gidx[r] : r of g[., ldg] (a per-centre gradient
// is broadcast to the centre's edge rows through gidx = ic).  dz[r, 0:Cpad] (0 in the pad and on invalid rows).
// NORM: the column sums of dy = dL/dLN-output and of dy * xhat are dbeta and dgamma: a workgroup takes RN_BWD_ROWS rows
// (one per wave: taking 16 or 64 rows per workgroup, a wave looping over its share, left too few loads in flight and ran slower), keeps the two sums of its rows in registers and leaves ONE partial row per
// workgroup: t_dy[blk, c], t_dyx[blk, c], blk < rownorm_bwd_blocks(rows) (summed by gn_colsum: fixed order).  Writing
// the per-row terms and reading them back was 40 % of this kernel's traffic plus two full passes of the column sum.
constexpr int RN_BWD_ROWS = 4;
int rownorm_bwd_blocks(long long rows) { return (int)((rows + RN_BWD_ROWS - 1) / RN_BWD_ROWS); }
template <bool NORM, int ACT, int NK>
__global__ __launch_bounds__(256) void rownorm_act_bwd_kernel(
    const float* __restrict__ g, long long ldg, const int* __restrict__ gidx,
    const float* __restrict__ z, long long ldz, int C, const int* __restrict__ valid,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ stats,
    float* __restrict__ dz, long long lddz, int Cpad, float* __restrict__ t_dy, float* __restrict__ t_dyx, long long rows,
    __bf16* __restrict__ dz16, long long lddz16, const int* __restrict__ argrow, int z_lowp)
{   // argrow (with gidx): max aggregation upstream - g[gidx[r], c] reaches row r only if argrow[gidx[r], c] == r
    // z_lowp bit 0: z holds bf16 values (a pre-activation kept in bf16, or an activation output whose sign stands in for the
    // pre-activation's); bit 1: g holds bf16 values
    constexpr int RPB = NORM ? RN_BWD_ROWS : 4;        // rows per workgroup
    __shared__ float red[NORM ? 4 : 1][2][NORM ? RN_MAXC : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float sdy[NK], sdyx[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) { sdy[k] = 0.0f; sdyx[k] = 0.0f; }
    for (int it = 0; it < RPB / 4; ++it) {
        const long long r = (long long)blockIdx.x * RPB + wave + 4 * it;
        if (r >= rows) break;
        const bool ok = !valid || valid[r] >= 0;
        const long long gr = gidx ? (long long)gidx[r] : r;
        float mean = 0.0f, rstd = 1.0f;
        if constexpr (NORM) { mean = stats[2 * r]; rstd = stats[2 * r + 1]; }
        float xh[NK], dy[NK];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            xh[k] = 0.0f; dy[k] = 0.0f;
            if (ok && c < C) {
                const float zz = ld_f32_or_bf16(z, r * ldz + c, (z_lowp & 1) != 0);
                float y = zz;
                if constexpr (NORM) { xh[k] = (zz - mean) * rstd; y = xh[k] * gamma[c] + beta[c]; }
                float gv = ld_f32_or_bf16(g, gr * ldg + c, (z_lowp & 2) != 0);
                if (argrow && argrow[gr * C + c] != (int)r) gv = 0.0f;
                dy[k] = gv * act_grad<ACT>(y);
                if constexpr (NORM) {
                    const float dxh = dy[k] * gamma[c];
                    s1 += dxh;
                    s2 += dxh * xh[k];
                }
            }
        }
        if constexpr (NORM) { s1 = wave_sum(s1) / (float)C; s2 = wave_sum(s2) / (float)C; }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            if (c < Cpad) {
                float o = 0.0f;
                if (ok && c < C) {
                    if constexpr (NORM) o = rstd * (dy[k] * gamma[c] - s1 - xh[k] * s2);
                    else o = dy[k];
                }
                if (dz) dz[r * lddz + c] = o;
                if (dz16) dz16[r * lddz16 + c] = (__bf16)o;
            }
            if constexpr (NORM) { sdy[k] += dy[k]; sdyx[k] += dy[k] * xh[k]; }
        }
    }
    if constexpr (NORM) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = lane + 64 * k;
            if (c < C) { red[wave][0][c] = sdy[k]; red[wave][1][c] = sdyx[k]; }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) {
            t_dy[(long long)blockIdx.x * C + c] = (red[0][0][c] + red[1][0][c]) + (red[2][0][c] + red[3][0][c]);
            t_dyx[(long long)blockIdx.x * C + c] = (red[0][1][c] + red[1][1][c]) + (red[2][1][c] + red[3][1][c]);
        }
    }
}

// out[i, c] = sum_{s < S} m[i*S + s, c]   (then the overflow rows are added by slot_sum_ovf_kernel)
__global__ __launch_bounds__(256) void slot_sum_kernel(const float* __restrict__ m, long long ldm, int C, int N, int S,
                                                       float* __restrict__ out, long long ldo) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / C), c = (int)(t % C);
    if (i >= N) return;
    float s = 0.0f;
    for (int k = 0; k < S; ++k) s += m[((long long)i * S + k) * ldm + c];
    out[(long long)i * ldo + c] = s;
}
__global__ __launch_bounds__(256) void slot_sum_ovf_kernel(const float* __restrict__ m, long long ldm, int C, EdgeGraph g,
                                                           int S, float* __restrict__ out, long long ldo) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int q = (int)(t / C), c = (int)(t % C);
    if (!g.ovf_cnt || q >= *g.ovf_cnt) return;
    out[(long long)g.ovf_centre[q] * ldo + c] += m[((long long)g.N * S + q) * ldm + c];    // <= 1 overflow row per centre
}

// ---------------------------------------------------------------- aggregation over a centre's edge rows
// aggr: 0 = add, 1 = mean (sum / number of edges), 2 = max (first occurrence; centres without edges -> 0).
// rows of centre i: i*S .. i*S+S-1 plus its overflow row N*S + q (ovf_of[i] = q or -1).  jc[row] < 0 = no edge.
// argrow[i, c] (aggr = max): the row that supplied the maximum (-1: none).
__global__ __launch_bounds__(256) void slot_reduce_kernel(const float* __restrict__ m, long long ldm, int C, int N, int S,
                                                          const int* __restrict__ jc, const int* __restrict__ ovf_row,
                                                          int aggr, float* __restrict__ out, long long ldo,
                                                          int* __restrict__ argrow, int post_act) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / C), c = (int)(t % C);
    if (i >= N) return;
    float acc = aggr == 2 ? -3.0e38f : 0.0f;
    int arg = -1, cnt = 0;
    for (int k = 0; k <= S; ++k) {
        long long row;
        if (k < S) row = (long long)i * S + k;
        else { const int q = ovf_row ? ovf_row[i] : -1; if (q < 0) break; row = (long long)N * S + q; }
        if (jc[row] < 0) continue;
        const float v = m[row * ldm + c];
        ++cnt;
        if (aggr == 2) { if (v > acc) { acc = v; arg = (int)row; } }
        else acc += v;
    }
    if (aggr == 1) acc = cnt > 0 ? acc / (float)cnt : 0.0f;
    if (aggr == 2 && arg < 0) acc = 0.0f;
    // a strictly increasing activation commutes with max (same value, same arg row): applied to the N x C result
    // instead of the N*S x C edge rows
    if (post_act == 2 && arg >= 0) acc = act_fwd<2>(acc);
    out[(long long)i * ldo + c] = acc;
    if (argrow) argrow[(long long)i * C + c] = arg;
}
// ovf_row[i] = index q of centre i's overflow row, -1 if none
__global__ __launch_bounds__(256) void ovf_row_kernel(EdgeGraph g, int* __restrict__ ovf_row) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < g.N) ovf_row[i] = -1;
}
__global__ __launch_bounds__(256) void ovf_row_fill_kernel(EdgeGraph g, int* __restrict__ ovf_row) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (g.ovf_cnt && q < *g.ovf_cnt) ovf_row[g.ovf_centre[q]] = q;
}
// g_rows[r, c] = d(loss)/d m[r, c] given gout[N, C]: add -> gout[ic]; mean -> gout[ic] / edges(ic);
// max -> gout[ic] only on the arg row.  Rows without an edge -> 0.  deg[i] = number of edges of centre i.
__global__ __launch_bounds__(256) void slot_reduce_bwd_kernel(const float* __restrict__ gout, long long ldg, int C,
                                                              const int* __restrict__ ic, const int* __restrict__ jc,
                                                              long long rows, int aggr, const int* __restrict__ deg,
                                                              const int* __restrict__ argrow, float* __restrict__ grows,
                                                              long long ldr, int Cpad) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long r = t / Cpad;
    const int c = (int)(t % Cpad);
    if (r >= rows) return;
    float v = 0.0f;
    if (c < C && jc[r] >= 0) {
        const int i = ic[r];
        const float go = gout[(long long)i * ldg + c];
        if (aggr == 0) v = go;
        else if (aggr == 1) v = go / (float)max(deg[i], 1);
        else v = (argrow[(long long)i * C + c] == (int)r) ? go : 0.0f;
    }
    grows[r * ldr + c] = v;
}
__global__ __launch_bounds__(256) void centre_degree_kernel(const int* __restrict__ jc, int N, int S,
                                                            const int* __restrict__ ovf_row, int* __restrict__ deg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int d = 0;
    for (int k = 0; k < S; ++k) d += jc[(long long)i * S + k] >= 0;
    if (ovf_row && ovf_row[i] >= 0) d += jc[(long long)N * S + ovf_row[i]] >= 0;
    deg[i] = d;
}

}  // namespace gn

// =============================================================== launchers
namespace gn {

static inline unsigned gblocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

hipError_t launch_edge_rows(const EdgeGraph& g, int S, int* ic, int* jc, hipStream_t st) {
    const long long rows = (long long)g.N * S + g.N;
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(edge_rows_kernel, dim3(gblocks(rows, 256)), dim3(256), 0, st, g, S, ic, jc, rows);
    return hipGetLastError();
}
// deg: [N] scratch; row_ptr: [N + 1]; tmp: scan scratch (gn_scan_tmp_ints(N)); ic / jc: [N * K + N] (capacity)
hipError_t launch_scan(const int* in, int* out, int n, int* tmp, int* total, hipStream_t st);      // graph.hip
hipError_t launch_rows_compact(const EdgeGraph& g, const int* ovf, int* deg, int* tmp, int* row_ptr, int* ic, int* jc, hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    const long long cap = (long long)g.N * g.K + g.N;
    hipError_t e = hipMemsetAsync(ic, 0, sizeof(int) * (size_t)cap, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(jc, 0xff, sizeof(int) * (size_t)cap, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rows_degree_kernel, dim3(gblocks(g.N, 256)), dim3(256), 0, st, g, ovf, deg);
    e = launch_scan(deg, row_ptr, g.N, tmp, row_ptr + g.N, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(rows_compact_fill_kernel, dim3(gblocks(g.N, 256)), dim3(256), 0, st, g, ovf, row_ptr, ic, jc);
    return hipGetLastError();
}
hipError_t launch_segment_rows_sum(const float* m, long long ldm, int C, int N, const int* row_ptr, float* out, long long ldo,
                                   int m_lowp, hipStream_t st) {
    if (N == 0) return hipSuccess;
    if (C < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(segment_rows_sum_kernel, dim3(gblocks((long long)N * C, 256)), dim3(256), 0, st, m, ldm, C, N, row_ptr, out, ldo, m_lowp);
    return hipGetLastError();
}
hipError_t launch_rev_rows_compact(const EdgeGraph& g, int S, const int* row_ptr, const int* rev_ptr, const int* rev_rows, int* out,
                                   hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    const long long cap = (long long)g.N * g.K + g.N;
    hipLaunchKernelGGL(rev_rows_compact_kernel, dim3(gblocks(cap, 256)), dim3(256), 0, st, g, S, row_ptr, rev_ptr, rev_rows, out);
    return hipGetLastError();
}
hipError_t launch_edge_gather_pre(const float* PQ, int H1p, const int* ic, const int* jc, long long rows, int act,
                                  void* pre, int pre_lowp, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    if ((H1p & 3) || (pre_lowp && (H1p & 7)) || (act != 2 && act != 3)) return hipErrorInvalidValue;
    const dim3 grid(gblocks(rows * (H1p >> 2), 256)), block(256);
#define GN_GP(ACT, T) hipLaunchKernelGGL((edge_gather_pre_kernel<ACT, T>), grid, block, 0, st, PQ, H1p, ic, jc, rows, (T*)pre)
    if (act == 2) { if (pre_lowp) GN_GP(2, __bf16); else GN_GP(2, float); }
    else { if (pre_lowp) GN_GP(3, __bf16); else GN_GP(3, float); }
#undef GN_GP
    return hipGetLastError();
}
hipError_t launch_rownorm_act_fwd(const float* z, long long ldz, int C, const int* valid, const float* gamma,
                                  const float* beta, float eps, int act, float* a, long long lda, int Cpad, float* stats,
                                  long long rows, void* a16, long long lda16, int z_lowp, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    if (C < 1 || Cpad < C || Cpad > RN_MAXC || act < 0 || act > 3 || ((gamma != nullptr) != (beta != nullptr)))
        return hipErrorInvalidValue;
    const dim3 grid(gblocks(rows, 4)), block(256);
    const bool norm = gamma != nullptr;
    const int nk = (Cpad + 63) / 64;
#define GN_RN_FWD_K(NRM, ACT, NK_) hipLaunchKernelGGL((rownorm_act_fwd_kernel<NRM, ACT, NK_>), grid, block, 0, st, z, ldz, C, valid, gamma, beta, eps, a, lda, Cpad, stats, rows, (__bf16*)a16, lda16, z_lowp)
#define GN_RN_FWD(NRM, ACT) do { if (nk <= 2) GN_RN_FWD_K(NRM, ACT, 2); else if (nk <= 4) GN_RN_FWD_K(NRM, ACT, 4); else if (nk <= 6) GN_RN_FWD_K(NRM, ACT, 6); else GN_RN_FWD_K(NRM, ACT, 8); } while (0)
    if (norm) { if (act == 0) GN_RN_FWD(true, 0); else if (act == 1) GN_RN_FWD(true, 1); else if (act == 2) GN_RN_FWD(true, 2); else GN_RN_FWD(true, 3); }
    else { if (act == 0) GN_RN_FWD(false, 0); else if (act == 1) GN_RN_FWD(false, 1); else if (act == 2) GN_RN_FWD(false, 2); else GN_RN_FWD(false, 3); }
#undef GN_RN_FWD
#undef GN_RN_FWD_K
    return hipGetLastError();
}
hipError_t launch_rownorm_act_bwd(const float* g, long long ldg, const int* gidx, const float* z, long long ldz, int C,
                                  const int* valid, const float* gamma, const float* beta, const float* stats, int act,
                                  float* dz, long long lddz, int Cpad, float* t_dy, float* t_dyx, long long rows,
                                  void* dz16, long long lddz16, const int* argrow, int z_lowp,
                                  hipStream_t st) {
    if (rows == 0) return hipSuccess;
    const bool norm = gamma != nullptr;
    if (C < 1 || Cpad < C || Cpad > RN_MAXC || act < 0 || act > 3 || (norm && (!beta || !stats || !t_dy || !t_dyx)) ||
        (argrow && !gidx))
        return hipErrorInvalidValue;
    const dim3 grid(norm ? rownorm_bwd_blocks(rows) : gblocks(rows, 4)), block(256);
    const int nk = (Cpad + 63) / 64;
#define GN_RN_BWD_K(NRM, ACT, NK_) hipLaunchKernelGGL((rownorm_act_bwd_kernel<NRM, ACT, NK_>), grid, block, 0, st, g, ldg, gidx, z, ldz, C, valid, gamma, beta, stats, dz, lddz, Cpad, t_dy, t_dyx, rows, (__bf16*)dz16, lddz16, argrow, z_lowp)
#define GN_RN_BWD(NRM, ACT) do { if (nk <= 2) GN_RN_BWD_K(NRM, ACT, 2); else if (nk <= 4) GN_RN_BWD_K(NRM, ACT, 4); else if (nk <= 6) GN_RN_BWD_K(NRM, ACT, 6); else GN_RN_BWD_K(NRM, ACT, 8); } while (0)
    if (norm) { if (act == 0) GN_RN_BWD(true, 0); else if (act == 1) GN_RN_BWD(true, 1); else if (act == 2) GN_RN_BWD(true, 2); else GN_RN_BWD(true, 3); }
    else { if (act == 0) GN_RN_BWD(false, 0); else if (act == 1) GN_RN_BWD(false, 1); else if (act == 2) GN_RN_BWD(false, 2); else GN_RN_BWD(false, 3); }
#undef GN_RN_BWD
#undef GN_RN_BWD_K
    return hipGetLastError();
}
// ovf_row, deg: int32[N] outputs (per graph, reusable); argrow: int32[N*C] output for aggr = max (else null)
hipError_t launch_slot_reduce(const float* m, long long ldm, int C, const EdgeGraph& g, int S, const int* jc, int aggr,
                              float* out, long long ldo, int* ovf_row, int* deg, int* argrow, int post_act,
                              hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    if (aggr < 0 || aggr > 2 || (aggr == 2 && !argrow) || !ovf_row || !deg) return hipErrorInvalidValue;
    if (post_act != 3 && !(post_act == 2 && aggr == 2)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ovf_row_kernel, dim3(gblocks(g.N, 256)), dim3(256), 0, st, g, ovf_row);
    if (g.ovf_cnt) hipLaunchKernelGGL(ovf_row_fill_kernel, dim3(gblocks(g.N, 256)), dim3(256), 0, st, g, ovf_row);
    hipLaunchKernelGGL(centre_degree_kernel, dim3(gblocks(g.N, 256)), dim3(256), 0, st, jc, g.N, S, ovf_row, deg);
    hipLaunchKernelGGL(slot_reduce_kernel, dim3(gblocks((long long)g.N * C, 256)), dim3(256), 0, st, m, ldm, C, g.N, S, jc,
                       ovf_row, aggr, out, ldo, argrow, post_act);
    return hipGetLastError();
}
hipError_t launch_slot_reduce_bwd(const float* gout, long long ldg, int C, const int* ic, const int* jc, long long rows,
                                  int aggr, const int* deg, const int* argrow, float* grows, long long ldr, int Cpad,
                                  hipStream_t st) {
    if (rows == 0) return hipSuccess;
    if (aggr < 0 || aggr > 2 || Cpad < C || (aggr == 1 && !deg) || (aggr == 2 && !argrow)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_reduce_bwd_kernel, dim3(gblocks(rows * Cpad, 256)), dim3(256), 0, st, gout, ldg, C, ic, jc, rows,
                       aggr, deg, argrow, grows, ldr, Cpad);
    return hipGetLastError();
}
// y[r, c] = (res ? res[r, c] : 0) + (keep(r, c) ? x[r, c] * inv : 0)   -- torch.nn.Dropout (+ residual add) and,
// applied to a gradient with the same seed, its backward.  x / y fp32 or bf16 (in place allowed), res fp32.
template <typename XT, typename YT>
__global__ __launch_bounds__(256) void dropout_kernel(const XT* __restrict__ x, long long ldx, const float* __restrict__ res,
                                                      long long ldres, YT* __restrict__ y, long long ldy, long long rows,
                                                      int cols, Drop dr) {
    const int c4n = cols >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * c4n) return;
    const long long r = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    const float4 v = load4<XT>(x + r * ldx + c);
    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = gn_keep(dr.seed, (unsigned)r, (unsigned)(c + j), dr.thresh) ? o[j] * dr.inv : 0.0f;
    if (res) {
        const float4 q = *reinterpret_cast<const float4*>(res + r * ldres + c);
        o[0] += q.x; o[1] += q.y; o[2] += q.z; o[3] += q.w;
    }
    store4<YT>(y + r * ldy + c, o[0], o[1], o[2], o[3]);
}

hipError_t launch_dropout(const void* x, long long ldx, int x_lowp, const float* res, long long ldres, void* y, long long ldy,
                          int y_lowp, long long rows, int cols, unsigned seed, unsigned thresh, hipStream_t st) {
    if (rows == 0 || cols == 0) return hipSuccess;
    if ((cols & 3) || (ldx & 3) || (ldy & 3) || (res && (ldres & 3))) return hipErrorInvalidValue;
    Drop dr;
    dr.seed = seed; dr.thresh = thresh; dr.inv = (float)(1.0 / (1.0 - (double)thresh / 4294967296.0));
    const dim3 grid(gblocks(rows * (cols >> 2), 256)), block(256);
    if (x_lowp && y_lowp) hipLaunchKernelGGL((dropout_kernel<__bf16, __bf16>), grid, block, 0, st, (const __bf16*)x, ldx, res, ldres, (__bf16*)y, ldy, rows, cols, dr);
    else if (x_lowp) hipLaunchKernelGGL((dropout_kernel<__bf16, float>), grid, block, 0, st, (const __bf16*)x, ldx, res, ldres, (float*)y, ldy, rows, cols, dr);
    else if (y_lowp) hipLaunchKernelGGL((dropout_kernel<float, __bf16>), grid, block, 0, st, (const float*)x, ldx, res, ldres, (__bf16*)y, ldy, rows, cols, dr);
    else hipLaunchKernelGGL((dropout_kernel<float, float>), grid, block, 0, st, (const float*)x, ldx, res, ldres, (float*)y, ldy, rows, cols, dr);
    return hipGetLastError();
}
// ------------------------------------------------------------------------------ BatchNorm1d over edge rows
// torch.nn.BatchNorm1d inside an EdgeConv MLP (ParticleNeT, models/gnn/particlenet.py:172-198) normalises every
// column over ALL edges of the batch; the edge-row tensors here also hold empty slots (valid[r] < 0), which take
// no part.  Forward: masked column sums of z and z^2 (BN_ROWS rows per workgroup, fixed-order partials) ->
// bn_finalize (mean, rstd, unbiased variance) -> bn_act_fwd.  Backward: masked column sums of dy and dy*xhat ->
// bn_act_bwd.  No atomics: two runs are bitwise identical.
constexpr int BN_ROWS = 256;
// part[blk][0:C] = sum_r f1, part[blk][C:2C] = sum_r f2 over the valid rows of the block, where
//   MODE 0: f1 = z, f2 = z^2;   MODE 1: f1 = dy, f2 = dy * xhat with dy = g * act'(xhat*gamma+beta)
template <int MODE, int ACT>
__global__ __launch_bounds__(256) void bn_sums_kernel(const float* __restrict__ z, long long ldz, long long rows, int C,
                                                      const int* __restrict__ valid, const float* __restrict__ g,
                                                      long long ldg, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ part) {
    __shared__ float red[2][4][RN_MAXC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long rbeg = (long long)blockIdx.x * BN_ROWS, rend = min(rows, rbeg + BN_ROWS);
    float s1[RN_PER], s2[RN_PER];
#pragma unroll
    for (int k = 0; k < RN_PER; ++k) { s1[k] = 0.0f; s2[k] = 0.0f; }
    for (long long r = rbeg + wave; r < rend; r += 4) {
        if (valid && valid[r] < 0) continue;
#pragma unroll
        for (int k = 0; k < RN_PER; ++k) {
            const int c = lane + 64 * k;
            if (c < C) {
                const float zz = z[r * ldz + c];
                if constexpr (MODE == 0) { s1[k] += zz; s2[k] = fmaf(zz, zz, s2[k]); }
                else {
                    const float xh = (zz - mean[c]) * rstd[c];
                    const float dy = g[r * ldg + c] * act_grad<ACT>(xh * gamma[c] + beta[c]);
                    s1[k] += dy; s2[k] = fmaf(dy, xh, s2[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < RN_PER; ++k) {
        const int c = lane + 64 * k;
        if (c < C) { red[0][wave][c] = s1[k]; red[1][wave][c] = s2[k]; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        part[(long long)blockIdx.x * 2 * C + c] = ((red[0][0][c] + red[0][1][c]) + red[0][2][c]) + red[0][3][c];
        part[(long long)blockIdx.x * 2 * C + C + c] = ((red[1][0][c] + red[1][1][c]) + red[1][2][c]) + red[1][3][c];
    }
}
// sums[0:C] = sum z, sums[C:2C] = sum z^2, n = *n_valid -> mean, rstd = 1/sqrt(var_biased + eps), var_unbiased
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ sums, const int* __restrict__ n_valid,
                                                          int C, float eps, float* __restrict__ mean,
                                                          float* __restrict__ rstd, float* __restrict__ var_unbiased) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double n = (double)max(*n_valid, 1);
    const double m = (double)sums[c] / n;
    double var = (double)sums[C + c] / n - m * m;
    if (var < 0.0) var = 0.0;
    mean[c] = (float)m;
    rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (var_unbiased) var_unbiased[c] = (float)(n > 1.0 ? var * n / (n - 1.0) : var);
}
// a[r, c] = act((z - mean) * rstd * gamma + beta); 0 on empty rows and pad columns
template <int ACT, typename OutT>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ z, long long ldz, long long rows, int C,
                                                         const int* __restrict__ valid, const float* __restrict__ mean,
                                                         const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, OutT* __restrict__ a, long long lda,
                                                         int Cpad) {
    const int c4n = Cpad >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * c4n) return;
    const long long r = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!valid || valid[r] >= 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C) o[j] = act_fwd<ACT>((z[r * ldz + c + j] - mean[c + j]) * rstd[c + j] * gamma[c + j] + beta[c + j]);
    }
    store4<OutT>(a + r * lda + c, o[0], o[1], o[2], o[3]);
}
// dz = gamma * rstd * (dy - sums[c]/n - xhat * sums[C+c]/n)   (training; eval: dz = gamma * rstd * dy, sums == null)
template <int ACT, typename OutT>
__global__ __launch_bounds__(256) void bn_act_bwd_kernel(const float* __restrict__ g, long long ldg, const float* __restrict__ z,
                                                         long long ldz, long long rows, int C, const int* __restrict__ valid,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ sums, const int* __restrict__ n_valid,
                                                         OutT* __restrict__ dz, long long lddz, int Cpad) {
    const int c4n = Cpad >> 2;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * c4n) return;
    const long long r = idx / c4n;
    const int c = (int)(idx % c4n) * 4;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (!valid || valid[r] >= 0) {
        const float inv_n = sums ? 1.0f / (float)max(*n_valid, 1) : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < C) {
                const int cc = c + j;
                const float xh = (z[r * ldz + cc] - mean[cc]) * rstd[cc];
                const float dy = g[r * ldg + cc] * act_grad<ACT>(xh * gamma[cc] + beta[cc]);
                const float corr = sums ? (sums[cc] + xh * sums[C + cc]) * inv_n : 0.0f;
                o[j] = gamma[cc] * rstd[cc] * (dy - corr);
            }
    }
    store4<OutT>(dz + r * lddz + c, o[0], o[1], o[2], o[3]);
}

int bn_blocks(long long rows) { return (int)((rows + BN_ROWS - 1) / BN_ROWS); }
hipError_t launch_reduce_slabs(const float* slab, int nslab, long long count, float* out, int accum, hipStream_t st);

// mode 0: forward moments of z; mode 1: backward sums (dbeta = sums[0:C], dgamma = sums[C:2C]).  part: bn_blocks*2C
hipError_t launch_bn_sums(int mode, int act, const float* z, long long ldz, long long rows, int C, const int* valid,
                          const float* g, long long ldg, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, float* part, float* sums, hipStream_t st) {
    if (C < 1 || C > RN_MAXC || (mode != 0 && mode != 1) || act < 0 || act > 3) return hipErrorInvalidValue;
    const int nb = bn_blocks(rows > 0 ? rows : 1);
    const dim3 grid(nb), block(256);
    if (mode == 0) hipLaunchKernelGGL((bn_sums_kernel<0, 3>), grid, block, 0, st, z, ldz, rows, C, valid, g, ldg, mean, rstd, gamma, beta, part);
    else {
#define GN_BNS(A) hipLaunchKernelGGL((bn_sums_kernel<1, A>), grid, block, 0, st, z, ldz, rows, C, valid, g, ldg, mean, rstd, gamma, beta, part)
        if (act == 0) GN_BNS(0); else if (act == 1) GN_BNS(1); else if (act == 2) GN_BNS(2); else GN_BNS(3);
#undef GN_BNS
    }
    return launch_reduce_slabs(part, nb, 2ll * C, sums, 0, st);
}
hipError_t launch_bn_finalize(const float* sums, const int* n_valid, int C, float eps, float* mean, float* rstd,
                              float* var_unbiased, hipStream_t st) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(gblocks(C, 256)), dim3(256), 0, st, sums, n_valid, C, eps, mean, rstd, var_unbiased);
    return hipGetLastError();
}
hipError_t launch_bn_act_fwd(const float* z, long long ldz, long long rows, int C, const int* valid, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, int act, void* a, long long lda,
                             int Cpad, int a_lowp, hipStream_t st) {
    if (rows == 0) return hipSuccess;
    if (C < 1 || Cpad < C || (Cpad & 3) || (a_lowp && (lda & 3)) || act < 0 || act > 3) return hipErrorInvalidValue;
    const dim3 grid(gblocks(rows * (Cpad >> 2), 256)), block(256);
#define GN_BNF(A, T) hipLaunchKernelGGL((bn_act_fwd_kernel<A, T>), grid, block, 0, st, z, ldz, rows, C, valid, mean, rstd, gamma, beta, (T*)a, lda, Cpad)
#define GN_BNF2(A) { if (a_lowp) GN_BNF(A, __bf16); else GN_BNF(A, float); }
    if (act == 0) GN_BNF2(0) else if (act == 1) GN_BNF2(1) else if (act == 2) GN_BNF2(2) else GN_BNF2(3)
#undef GN_BNF2
#undef GN_BNF
    return hipGetLastError();
}
hipError_t launch_bn_act_bwd(const float* g, long long ldg, const float* z, long long ldz, long long rows, int C,
                             const int* valid, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const float* sums, const int* n_valid, int act, void* dz, long long lddz, int Cpad, int dz_lowp,
                             hipStream_t st) {
    if (rows == 0) return hipSuccess;
    if (C < 1 || Cpad < C || (Cpad & 3) || act < 0 || act > 3 || (sums && !n_valid)) return hipErrorInvalidValue;
    const dim3 grid(gblocks(rows * (Cpad >> 2), 256)), block(256);
#define GN_BNB(A, T) hipLaunchKernelGGL((bn_act_bwd_kernel<A, T>), grid, block, 0, st, g, ldg, z, ldz, rows, C, valid, mean, rstd, gamma, beta, sums, n_valid, (T*)dz, lddz, Cpad)
#define GN_BNB2(A) { if (dz_lowp) GN_BNB(A, __bf16); else GN_BNB(A, float); }
    if (act == 0) GN_BNB2(0) else if (act == 1) GN_BNB2(1) else if (act == 2) GN_BNB2(2) else GN_BNB2(3)
#undef GN_BNB2
#undef GN_BNB
    return hipGetLastError();
}

hipError_t launch_slot_sum(const float* m, long long ldm, int C, const EdgeGraph& g, int S, float* out, long long ldo,
                           hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    hipLaunchKernelGGL(slot_sum_kernel, dim3(gblocks((long long)g.N * C, 256)), dim3(256), 0, st, m, ldm, C, g.N, S, out, ldo);
    if (g.ovf_cnt)
        hipLaunchKernelGGL(slot_sum_ovf_kernel, dim3(gblocks((long long)g.N * C, 256)), dim3(256), 0, st, m, ldm, C, g, S,
                           out, ldo);
    return hipGetLastError();
}

}  // namespace gn
