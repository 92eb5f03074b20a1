// graphnet_amd/csrc/rnn.hip — ragged GRU recurrence over DOM time series (gfx950), fp32 in both compute modes.
//
//   Node_RNN (models/rnn/node_rnn.py:91-136) runs torch.nn.GRU over ~10^5 series of 1 to a few hundred rows per batch and
//   keeps h_n of layer 0.  Series s owns rows series_ptr[s] .. series_ptr[s+1] of xs[T, I]; gate order r, z, n; h starts at 0.
//
//   gru_fwd_kernel<HP>   persistent waves, one series per wave at a time, lane j = hidden unit j.  The three rows j, H + j,
//                        2H + j of W_hh stay in registers for the life of the wave (3 * HP floats), W_ih is staged once per
//                        workgroup in LDS, transposed, so that lane j reads consecutive words.  h travels between lanes by
//                        v_readlane: no LDS exchange, so the waves of a workgroup never wait for each other after the staging
//                        barrier (their series differ in length).  A series' first row skips the W_hh product (h = 0).
//                        Saved for the backward, as planes [T, H]: r, z, n, gh_n, h_prev (zeros on a series' first row).
//   gru_bwd_kernel<HP>   the same walk from a series' last row to its first with column j of W_hh in registers; writes the
//                        pre-activation gradients dgi[T, 3H] (input side) and dgh[T, 3H] (hidden side; they differ in the n
//                        block by the factor r) and a copy of xs padded to a multiple of four columns.
//   The parameter gradients are dgi^T xs, colsum(dgi), dgh^T h_prev, colsum(dgh) by launch_gemm_tn in GN_MODE_F32: sums in a
//   fixed order, no float atomics anywhere, so two runs agree bit for bit.
//
//   dom_summary_kernel   one thread per series: its first row, with the charge column replaced by asinhf((5 * s) / 5), s the
//                        fp32 sum of the series' charges in row order.
#include "launchers.hpp"

namespace gn {

constexpr int GRU_NT = 256;            // 4 waves: each holds up to 192 weights per lane, so at most 2 waves fit a SIMD
constexpr int GRU_WAVES = GRU_NT / 64;
constexpr int GRU_HMAX = 64, GRU_IMAX = 32;

int gru_supported(int I, int H) { return I >= 1 && I <= GRU_IMAX && H >= 4 && H <= GRU_HMAX && H % 4 == 0 ? 1 : 0; }
long long gru_saved_floats(int T, int H) { return 5ll * T * H; }
static int gru_ipad(int I) { return (I + 3) / 4 * 4; }

__device__ __forceinline__ float gru_lane(float v, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ float gru_sigmoid(float v) { return 1.0f / (1.0f + __expf(-v)); }

template <int HP>
__global__ __launch_bounds__(GRU_NT) void gru_fwd_kernel(
    const float* __restrict__ xs, long long ldx, int T, int I, const int* __restrict__ series_ptr, int M, int H,
    const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
    const float* __restrict__ b_hh, float* __restrict__ out, float* __restrict__ saved)
{
    __shared__ float wih_t[GRU_IMAX * 3 * HP];              // [i][g * H + j]
    const int tid = (int)threadIdx.x, j = tid & 63;
    const int H3 = 3 * H;
    for (int idx = tid; idx < I * H3; idx += GRU_NT) {
        const int i = idx / H3, c = idx - i * H3;
        wih_t[idx] = w_ih[(long long)c * I + i];
    }
    const bool live = j < H;
    float w[3][HP];
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int k = 0; k < HP; ++k) w[g][k] = (live && k < H) ? w_hh[(long long)(g * H + j) * H + k] : 0.0f;
    float bi[3], bh[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) { bi[g] = live ? b_ih[g * H + j] : 0.0f; bh[g] = live ? b_hh[g * H + j] : 0.0f; }
    __syncthreads();

    const long long TH = (long long)T * H;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = (int)gridDim.x * GRU_WAVES;
    for (int s = (int)blockIdx.x * GRU_WAVES + wave; s < M; s += stride) {
        const int t1 = min(series_ptr[s + 1], T), t0 = min(max(series_ptr[s], 0), t1);
        float h = 0.0f;
        for (int t = t0; t < t1; ++t) {
            float gi[3] = {bi[0], bi[1], bi[2]};
            const float* xr = xs + (long long)t * ldx;
            for (int i = 0; i < I; ++i) {
                const float xv = xr[i];
                const float* wr = wih_t + i * H3 + (live ? j : 0);
                gi[0] += wr[0] * xv; gi[1] += wr[H] * xv; gi[2] += wr[2 * H] * xv;
            }
            float gh[3] = {bh[0], bh[1], bh[2]};
            if (t > t0) {
#pragma unroll
                for (int k = 0; k < HP; ++k) {
                    const float hk = gru_lane(h, k);
                    gh[0] += w[0][k] * hk; gh[1] += w[1][k] * hk; gh[2] += w[2][k] * hk;
                }
            }
            const float r = gru_sigmoid(gi[0] + gh[0]);
            const float z = gru_sigmoid(gi[1] + gh[1]);
            const float n = tanhf(gi[2] + r * gh[2]);
            if (saved && live) {
                float* sv = saved + (long long)t * H + j;
                sv[0] = r; sv[TH] = z; sv[2 * TH] = n; sv[3 * TH] = gh[2]; sv[4 * TH] = h;
            }
            h = live ? (1.0f - z) * n + z * h : 0.0f;
        }
        if (live) out[(long long)s * H + j] = h;
    }
}

template <int HP>
__global__ __launch_bounds__(GRU_NT) void gru_bwd_kernel(
    const float* __restrict__ dout, const float* __restrict__ saved, const float* __restrict__ xs, long long ldx, int T, int I,
    int Ip, const int* __restrict__ series_ptr, int M, int H, const float* __restrict__ w_hh, float* __restrict__ dgi,
    float* __restrict__ dgh, float* __restrict__ xs_pad)
{
    const int tid = (int)threadIdx.x, j = tid & 63;
    const bool live = j < H;
    float wt[3][HP];                                        // column j of W_hh: wt[g][k] = W_hh[g * H + k][j]
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int k = 0; k < HP; ++k) wt[g][k] = (live && k < H) ? w_hh[(long long)(g * H + k) * H + j] : 0.0f;

    const long long TH = (long long)T * H;
    const int H3 = 3 * H;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = (int)gridDim.x * GRU_WAVES;
    for (int s = (int)blockIdx.x * GRU_WAVES + wave; s < M; s += stride) {
        const int t1 = min(series_ptr[s + 1], T), t0 = min(max(series_ptr[s], 0), t1);
        float dh = live ? dout[(long long)s * H + j] : 0.0f;
        for (int t = t1 - 1; t >= t0; --t) {
            float r = 0.0f, z = 0.0f, n = 0.0f, ghn = 0.0f, hp = 0.0f;
            if (live) {
                const float* sv = saved + (long long)t * H + j;
                r = sv[0]; z = sv[TH]; n = sv[2 * TH]; ghn = sv[3 * TH]; hp = sv[4 * TH];
            }
            const float dn = dh * (1.0f - z);
            const float dan = dn * (1.0f - n * n);           // d pre-activation of n (input side)
            const float daz = dh * (hp - n) * z * (1.0f - z);
            const float dar = dan * ghn * r * (1.0f - r);
            const float dhn = dan * r;                       // d gh_n (hidden side)
            if (live) {
                float* gi = dgi + (long long)t * H3 + j;
                float* gh = dgh + (long long)t * H3 + j;
                gi[0] = dar; gi[H] = daz; gi[2 * H] = dan;
                gh[0] = dar; gh[H] = daz; gh[2 * H] = dhn;
            }
            if (j < Ip) xs_pad[(long long)t * Ip + j] = j < I ? xs[(long long)t * ldx + j] : 0.0f;
            if (t > t0) {
                float acc = dh * z;
#pragma unroll
                for (int k = 0; k < HP; ++k)
                    acc += wt[0][k] * gru_lane(dar, k) + wt[1][k] * gru_lane(daz, k) + wt[2][k] * gru_lane(dhn, k);
                dh = live ? acc : 0.0f;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dom_summary_kernel(
    const float* __restrict__ x, long long ldx, int F, int N, const int* __restrict__ series_ptr, int M, int charge_col,
    float* __restrict__ out, long long ldo)
{
#pragma clang fp contract(off)
    const int s = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (s >= M) return;
    const int t1 = min(series_ptr[s + 1], N), t0 = min(max(series_ptr[s], 0), t1);
    if (t0 >= t1) {
        for (int c = 0; c < F; ++c) out[(long long)s * ldo + c] = 0.0f;
        return;
    }
    float sum = 0.0f;
    for (int t = t0; t < t1; ++t) sum += x[(long long)t * ldx + charge_col];
    const float* r0 = x + (long long)t0 * ldx;
    for (int c = 0; c < F; ++c) out[(long long)s * ldo + c] = c == charge_col ? asinhf((5.0f * sum) / 5.0f) : r0[c];
}

static int gru_grid(int M) {
    const int want = (M + GRU_WAVES - 1) / GRU_WAVES;
    return want < 512 ? (want > 0 ? want : 1) : 512;        // 256 CUs x 2 resident workgroups
}

hipError_t launch_gru_series_fwd(const float* xs, long long ldx, int T, int I, const int* series_ptr, int M, int H,
                                 const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                                 float* saved, hipStream_t st) {
    if (!gru_supported(I, H)) return hipErrorNotSupported;
    if (M == 0) return hipSuccess;
    const dim3 grid((unsigned)gru_grid(M)), block(GRU_NT);
    if (H <= 16)
        hipLaunchKernelGGL(gru_fwd_kernel<16>, grid, block, 0, st, xs, ldx, T, I, series_ptr, M, H, w_ih, w_hh, b_ih, b_hh, out, saved);
    else if (H <= 32)
        hipLaunchKernelGGL(gru_fwd_kernel<32>, grid, block, 0, st, xs, ldx, T, I, series_ptr, M, H, w_ih, w_hh, b_ih, b_hh, out, saved);
    else
        hipLaunchKernelGGL(gru_fwd_kernel<64>, grid, block, 0, st, xs, ldx, T, I, series_ptr, M, H, w_ih, w_hh, b_ih, b_hh, out, saved);
    return hipGetLastError();
}

// work: [dgi T*3H][dgh T*3H][xs_pad T*Ip][slab parts*3H*max(Ip, H)][db_part max(parts, colsum blocks)*3H] floats
struct GruWork { long long dgi, dgh, xs_pad, slab, db_part, total; };
static GruWork gru_work_layout(int T, int I, int H) {
    const int Ip = gru_ipad(I), H3 = 3 * H;
    const int parts_i = gemm_tn_parts(0, T, H3, &Ip, 1), parts_h = gemm_tn_parts(0, T, H3, &H, 1);
    const int parts = parts_i > parts_h ? parts_i : parts_h;
    const int cb = colsum_blocks(T);
    GruWork L;
    L.dgi = 0;
    L.dgh = L.dgi + (long long)T * H3;
    L.xs_pad = L.dgh + (long long)T * H3;
    L.slab = L.xs_pad + (long long)T * Ip;
    L.db_part = L.slab + (long long)parts * H3 * (Ip > H ? Ip : H);
    L.total = L.db_part + (long long)(parts > cb ? parts : cb) * H3;
    return L;
}
long long gru_bwd_work_floats(int T, int I, int H) { return gru_work_layout(T, I, H).total; }

hipError_t launch_gru_series_bwd(const float* dout, const float* saved, const float* xs, long long ldx, int T, int I,
                                 const int* series_ptr, int M, int H, const float* w_hh, float* dw_ih, float* db_ih,
                                 float* dw_hh, float* db_hh, float* work, hipStream_t st) {
    if (!gru_supported(I, H)) return hipErrorNotSupported;
    const int Ip = gru_ipad(I), H3 = 3 * H;
    if (M == 0 || T == 0) {
        hipError_t e = hipMemsetAsync(dw_ih, 0, sizeof(float) * H3 * Ip, st);
        if (e == hipSuccess) e = hipMemsetAsync(dw_hh, 0, sizeof(float) * H3 * H, st);
        if (e == hipSuccess) e = hipMemsetAsync(db_ih, 0, sizeof(float) * H3, st);
        if (e == hipSuccess) e = hipMemsetAsync(db_hh, 0, sizeof(float) * H3, st);
        return e;
    }
    const GruWork L = gru_work_layout(T, I, H);
    float* dgi = work + L.dgi;
    float* dgh = work + L.dgh;
    float* xs_pad = work + L.xs_pad;
    const dim3 grid((unsigned)gru_grid(M)), block(GRU_NT);
    if (H <= 16)
        hipLaunchKernelGGL(gru_bwd_kernel<16>, grid, block, 0, st, dout, saved, xs, ldx, T, I, Ip, series_ptr, M, H, w_hh, dgi, dgh, xs_pad);
    else if (H <= 32)
        hipLaunchKernelGGL(gru_bwd_kernel<32>, grid, block, 0, st, dout, saved, xs, ldx, T, I, Ip, series_ptr, M, H, w_hh, dgi, dgh, xs_pad);
    else
        hipLaunchKernelGGL(gru_bwd_kernel<64>, grid, block, 0, st, dout, saved, xs, ldx, T, I, Ip, series_ptr, M, H, w_hh, dgi, dgh, xs_pad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    Segs x = {};
    x.nseg = 1; x.p[0] = xs_pad; x.ld[0] = Ip; x.width[0] = Ip; x.kpad[0] = Ip;
    e = launch_gemm_tn(0, dgi, 0, H3, H3, x, 0, T, work + L.slab, work + L.db_part, dw_ih, db_ih, 0, st);
    if (e != hipSuccess) return e;
    x.p[0] = saved + 4ll * T * H; x.ld[0] = H; x.width[0] = H; x.kpad[0] = H;
    return launch_gemm_tn(0, dgh, 0, H3, H3, x, 0, T, work + L.slab, work + L.db_part, dw_hh, db_hh, 0, st);
}

hipError_t launch_dom_series_summary(const float* x, long long ldx, int F, int N, const int* series_ptr, int M, int charge_col,
                                     float* out, long long ldo, hipStream_t st) {
    if (M == 0) return hipSuccess;
    hipLaunchKernelGGL(dom_summary_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, x, ldx, F, N, series_ptr, M,
                       charge_col, out, ldo);
    return hipGetLastError();
}

}  // namespace gn
