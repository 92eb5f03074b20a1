// graphnet_amd/csrc/edgeconv_norm.hip — fused edge MLP  Linear, LayerNorm, GELU, Linear, LayerNorm, GELU, sum over the
// centre's edges  (DynEdge with activation_layer="gelu", add_norm_layer=True: the one DeepIce embeds), on the compact edge
// rows of gn_rows_compact.  The row kernels of generic.hip keep pre1, a1, z2 and m as [E, H] tensors in HBM; here a workgroup
// owns a CENTRE-ALIGNED TILE of at most 64 edge rows with its full width, so both LayerNorm reductions and the per-centre
// sums happen inside the tile: no [E, H] tensor on the way forward (16 bytes of statistics per row), three on the way back.
//
// Tiles.  Centre i belongs to tile row_ptr[i] / (64 - K): the first rows of a tile's centres lie in a window of 64 - K rows
// and the last centre adds at most K more (a centre has at most K + 1 rows), so a tile has at most 64 rows, no centre
// straddles two tiles, and the plan is one independent decision per centre (edgeconv_norm_plan_kernel).  No atomics.
//
// One workgroup = 4 waves.  LDS (dynamic): region R0 holds, one after the other,
//     forward :  a1 [64][H1p] T  ->  z2 / m [64][H2] fp32
//     backward:  a1 [64][H1p] T  ->  z2 [64][H2] fp32 -> dz2 [64][H2] T  ->  da1 / dpre1 [64][H1p] fp32
// (T = the mode's MFMA operand type; rows padded by 16 bytes), region WC one 32-deep K chunk of the weight operand
// ([H2 or H1p rows][32] T, pitch TileCfg<T>::ROWB), reused at the end for the LayerNorm-gradient partial sums.
// The largest case (fp32 mode, H1p = 352, H2 = 256): R0 = 64 * 1424 = 91,136 bytes, WC = 352 * 144 = 50,688 bytes, 141,824 of the
// 163,840 bytes of a workgroup.  Accumulators: 64 x H2 over 4 waves = 2 x 2 tiles of 32 x 32 per wave (64 registers) in the
// forward GEMM, 2 x 3 (96 registers) in the backward one; the next weight chunk waits in at most 11 x 4 registers.
//
// Row phases (LayerNorm, GELU and their derivatives) run one wave per row with the column layout, the operation order and
// the wave sum of rownorm_act_fwd / _bwd_kernel (lane + 64 k), so the statistics are the row kernels' statistics.
#include "common.hpp"
#include "row_math.hpp"

namespace gn {

constexpr int EN_ROWS = 64;            // rows of a tile
constexpr int EN_NK1 = 6;              // columns per lane of an H1p-wide row: ceil(352 / 64)
constexpr int EN_NK2 = 4;              // of an H2-wide row: 256 / 64
constexpr int EN_MAXH1P = 352, EN_MAXH2 = 256;

bool edgeconv_norm_supported(int mode, int H1, int H2) {
    return (mode == 0 || mode == 1) && H1 >= 1 && (H1 + 31) / 32 * 32 <= EN_MAXH1P && H2 >= 32 && H2 % 32 == 0 && H2 <= EN_MAXH2;
}
int edgeconv_norm_tiles(int N, int K) {
    if (N < 0 || K < 1 || K > 32) return -1;
    return (int)(((long long)N * (K + 1)) / (EN_ROWS - K)) + 1;
}

// plan[t] = first centre of tile t, t <= ntiles (plan[ntiles] = N; tiles past the last edge are empty).  Thread i <= N fills
// the tiles that begin between centre i - 1's and centre i's.
__global__ __launch_bounds__(256) void edgeconv_norm_plan_kernel(const int* __restrict__ row_ptr, int N, int W, int ntiles,
                                                                 int* __restrict__ plan) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    const int b = i < N ? min(row_ptr[i] / W, ntiles - 1) : ntiles;
    const int pb = i > 0 ? min(row_ptr[i - 1] / W, ntiles - 1) : -1;
    for (int t = pb + 1; t <= b; ++t) plan[t] = i;
}

template <typename T> struct ENCfg {
    static constexpr int SZ = (int)sizeof(T);
    static constexpr int VPR = BK * SZ / 16;                         // 16-byte pieces of a weight row in one K chunk
    __host__ __device__ static int pitch_t(int cols) { return cols * SZ + 16; }      // operand tile row, bytes
    __host__ __device__ static int pitch_f(int cols) { return cols * 4 + 16; }       // fp32 tile row, bytes
    // backward: the dz2 operand tile shares the z2 tile's bytes when the pitches agree (fp32), else it follows it
    __host__ __device__ static int off_d(int H2) { return SZ == 4 ? 0 : EN_ROWS * pitch_f(H2); }
    static int r0_fwd(int H1p, int H2) { return EN_ROWS * max(pitch_t(H1p), pitch_f(H2)); }
    static int r0_bwd(int H1p, int H2) { return max(max(EN_ROWS * pitch_t(H1p), off_d(H2) + EN_ROWS * pitch_t(H2)), EN_ROWS * pitch_f(H1p)); }
    static int wc(int rows) { return rows * TileCfg<T>::ROWB; }
};

// ---------------------------------------------------------------- tile set-up: rows and centres
struct ENTile { int c0, c1, r0, nr; };
// cen[lr] = centre of local row lr.  A tile whose row count breaks the plan's bound is SKIPPED (treated as empty: out, dP and
// stats of its centres stay unwritten, no error is returned - include/graphnet_amd.h says so).  That takes a row_ptr that is
// not gn_rows_compact's (a centre with more than K + 1 rows); the guard is there so that no LDS row past the tile is written.
__device__ __forceinline__ ENTile en_tile(const int* __restrict__ plan, const int* __restrict__ row_ptr, int* cen) {
    ENTile t;
    t.c0 = plan[blockIdx.x]; t.c1 = plan[blockIdx.x + 1];
    t.r0 = t.c1 > t.c0 ? row_ptr[t.c0] : 0;
    t.nr = t.c1 > t.c0 ? row_ptr[t.c1] - t.r0 : 0;
    if (t.nr < 0 || t.nr > EN_ROWS) { t.nr = 0; t.c1 = t.c0; }
    for (int i = t.c0 + (int)threadIdx.x; i < t.c1; i += 256)
        for (int r = row_ptr[i]; r < row_ptr[i + 1]; ++r) cen[r - t.r0] = i;
    __syncthreads();
    return t;
}

// ---------------------------------------------------------------- GEMM of a tile: acc[64 x 32 TN] += A[64 x 32 nk] . Wp^T
// A: LDS operand tile (pitch pa bytes); Wp: packed weight [>= nw rows][Kp] of T, K contiguous; WC: the chunk buffer.  Wave w
// owns the 32-column blocks w, w + 4, ... < NB.  The next chunk is fetched into registers while the current one multiplies.
template <typename T, int MAXV>
__device__ __forceinline__ void en_w_load(u32x4 (&v)[MAXV], const T* __restrict__ Wp, int Kp, int nw, int kc) {
    constexpr int VPR = ENCfg<T>::VPR;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int idx = (int)threadIdx.x + 256 * u;
        if (idx < nw * VPR)
            v[u] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(Wp) +
                                                   ((size_t)(idx / VPR) * Kp + (size_t)kc * BK) * sizeof(T) + (idx % VPR) * 16);
    }
}
template <typename T, int MAXV>
__device__ __forceinline__ void en_w_store(const u32x4 (&v)[MAXV], unsigned char* WC, int nw) {
    constexpr int VPR = ENCfg<T>::VPR;
#pragma unroll
    for (int u = 0; u < MAXV; ++u) {
        const int idx = (int)threadIdx.x + 256 * u;
        if (idx < nw * VPR) *reinterpret_cast<u32x4*>(WC + (idx / VPR) * TileCfg<T>::ROWB + (idx % VPR) * 16) = v[u];
    }
}
template <typename T, int TN, int NWMAX>
__device__ __forceinline__ void en_gemm(const unsigned char* A, int pa, const T* __restrict__ Wp, int Kp, int nw, int nk,
                                        unsigned char* WC, f32x16 (&acc)[2][TN]) {
    constexpr int MAXV = (NWMAX * ENCfg<T>::VPR + 255) / 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int NB = nw / 32;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < TN; ++n) zero_acc(acc[m][n]);
    u32x4 st[MAXV];
    en_w_load<T, MAXV>(st, Wp, Kp, nw, 0);
    for (int kc = 0; kc < nk; ++kc) {
        __syncthreads();                         // the previous chunk has been read (first pass: the A tile is complete)
        en_w_store<T, MAXV>(st, WC, nw);
        __syncthreads();
        if (kc + 1 < nk) en_w_load<T, MAXV>(st, Wp, Kp, nw, kc + 1);
#pragma unroll
        for (int s = 0; s < TileCfg<T>::KSTEPS; ++s) {
            Frag<T> fa[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const unsigned char* p = A + (m * 32 + r) * pa + (kc * BK) * (int)sizeof(T) + s * 32 + h * 16;
                if constexpr (sizeof(T) == 4) fa[m].v = *reinterpret_cast<const f32x4*>(p);
                else fa[m].v = *reinterpret_cast<const bf16x8*>(p);
            }
#pragma unroll
            for (int n = 0; n < TN; ++n) {
                const int cb = wave + 4 * n;
                if (cb < NB) {
                    const Frag<T> fb = lds_frag<T>(WC, cb * 32 + r, s, h);
#pragma unroll
                    for (int m = 0; m < 2; ++m) mma(fa[m], fb, acc[m][n]);
                }
            }
        }
    }
    __syncthreads();                             // every wave is done with A and WC
}
// accumulators (+ bias) -> fp32 LDS tile dst (pitch pf bytes)
template <int TN>
__device__ __forceinline__ void en_acc_store(const f32x16 (&acc)[2][TN], int NB, const float* __restrict__ bias,
                                             unsigned char* dst, int pf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5;
#pragma unroll
    for (int n = 0; n < TN; ++n) {
        const int cb = wave + 4 * n;
        if (cb < NB) {
            const int col = cb * 32 + (lane & 31);
            const float b = bias ? bias[col] : 0.0f;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int q = 0; q < 16; ++q)
                    *reinterpret_cast<float*>(dst + (m * 32 + acc_row(q, h)) * pf + col * 4) = acc[m][n][q] + b;
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- row phases (one wave per row, 16 rows per wave)
// pre1 row = P[i] + Q[j] in the lane + 64 k layout; the centre's P row stays in registers while the centre does
__device__ __forceinline__ void en_gather(const float* __restrict__ PQ, int H1p, int H1, int i, int j, int& prev_i,
                                          float (&p)[EN_NK1], float (&v)[EN_NK1]) {
    const int lane = threadIdx.x & 63;
    if (i != prev_i) {
#pragma unroll
        for (int k = 0; k < EN_NK1; ++k) {
            const int c = lane + 64 * k;
            p[k] = c < H1 ? PQ[(long long)i * 2 * H1p + c] : 0.0f;
        }
        prev_i = i;
    }
#pragma unroll
    for (int k = 0; k < EN_NK1; ++k) {
        const int c = lane + 64 * k;
        v[k] = c < H1 ? p[k] + PQ[(long long)j * 2 * H1p + H1p + c] : 0.0f;
    }
}
// LayerNorm statistics of a row held as v[NK] (columns >= C hold 0): rownorm_act_fwd_kernel's two passes
template <int NK>
__device__ __forceinline__ void en_stats(const float (&v)[NK], int C, float eps, float& mean, float& rstd) {
    const int lane = threadIdx.x & 63;
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
}
// a1 rows of the tile into the LDS operand tile (and to a1g [rows, H1p] of T when given); rows nr..63 of the tile are zero.
// STATS: compute and store (mean1, rstd1) (forward), else read them (backward).
template <typename T, bool STATS>
__device__ __forceinline__ void en_rows_a1(const ENTile& t, const int* cen, const float* __restrict__ PQ, int H1p, int H1,
                                           const int* __restrict__ jc, const float* __restrict__ gamma1,
                                           const float* __restrict__ beta1, float eps, float* __restrict__ stats,
                                           unsigned char* A, int pa, T* __restrict__ a1g) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float p[EN_NK1], v[EN_NK1];
    int prev_i = -1;
    for (int it = 0; it < EN_ROWS / 4; ++it) {
        const int lr = wave * (EN_ROWS / 4) + it;
        if (lr >= t.nr) break;
        const long long r = (long long)t.r0 + lr;
        en_gather(PQ, H1p, H1, cen[lr], jc[r], prev_i, p, v);
        float mean, rstd;
        if constexpr (STATS) {
            en_stats<EN_NK1>(v, H1, eps, mean, rstd);
            if (lane == 0) { stats[4 * r] = mean; stats[4 * r + 1] = rstd; }
        } else {
            mean = stats[4 * r]; rstd = stats[4 * r + 1];
        }
#pragma unroll
        for (int k = 0; k < EN_NK1; ++k) {
            const int c = lane + 64 * k;
            if (c < H1p) {
                float o = 0.0f;
                if (c < H1) o = act_fwd<1>((v[k] - mean) * rstd * gamma1[c] + beta1[c]);
                *reinterpret_cast<T*>(A + lr * pa + c * (int)sizeof(T)) = from_f32<T>(o);
                if (a1g) a1g[r * H1p + c] = from_f32<T>(o);
            }
        }
    }
    for (int lr = t.nr + wave; lr < EN_ROWS; lr += 4)
#pragma unroll
        for (int k = 0; k < EN_NK1; ++k) {
            const int c = lane + 64 * k;
            if (c < H1p) *reinterpret_cast<T*>(A + lr * pa + c * (int)sizeof(T)) = from_f32<T>(0.0f);
        }
}
// out[i, c] = sum over centre i's rows of the fp32 LDS tile, ascending rows (gn_segment_rows_sum's order); no rows -> 0
template <typename OutT>
__device__ __forceinline__ void en_centre_sums(const ENTile& t, const int* __restrict__ row_ptr, const unsigned char* tile, int pf,
                                               int C, OutT* __restrict__ out, long long ldo) {
    const long long total = (long long)(t.c1 - t.c0) * C;
    for (long long idx = threadIdx.x; idx < total; idx += 256) {
        const int i = t.c0 + (int)(idx / C), c = (int)(idx % C);
        float s = 0.0f;
        for (int lr = row_ptr[i] - t.r0; lr < row_ptr[i + 1] - t.r0; ++lr) s += *reinterpret_cast<const float*>(tile + lr * pf + c * 4);
        out[(long long)i * ldo + c] = from_f32<OutT>(s);
    }
}

// ================================================================ forward
template <typename T>
__global__ __launch_bounds__(256) void edgeconv_norm_fwd_kernel(
    const float* __restrict__ PQ, int H1p, int H1, int H2, const int* __restrict__ row_ptr, const int* __restrict__ jc,
    const int* __restrict__ plan, const T* __restrict__ W2p, const float* __restrict__ b2, const float* __restrict__ gamma1,
    const float* __restrict__ beta1, const float* __restrict__ gamma2, const float* __restrict__ beta2, float eps,
    float* __restrict__ out, long long ldo, float* __restrict__ stats, int r0_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char en_lds[];
    __shared__ int cen[EN_ROWS];
    unsigned char* R0 = en_lds;
    unsigned char* WC = en_lds + r0_bytes;
    const ENTile t = en_tile(plan, row_ptr, cen);
    if (t.c1 <= t.c0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pa = ENCfg<T>::pitch_t(H1p), pz = ENCfg<T>::pitch_f(H2);

    en_rows_a1<T, true>(t, cen, PQ, H1p, H1, jc, gamma1, beta1, eps, stats, R0, pa, (T*)nullptr);
    f32x16 acc[2][2];
    en_gemm<T, 2, EN_MAXH2>(R0, pa, W2p, H1p, H2, H1p / BK, WC, acc);
    en_acc_store<2>(acc, H2 / 32, b2, R0, pz);                                   // z2 = a1 . W2^T + b2

    for (int it = 0; it < EN_ROWS / 4; ++it) {                                   // m = gelu(LN(z2)), in place
        const int lr = wave * (EN_ROWS / 4) + it;
        if (lr >= t.nr) break;
        const long long r = (long long)t.r0 + lr;
        float* zr = reinterpret_cast<float*>(R0 + lr * pz);
        float v[EN_NK2];
#pragma unroll
        for (int k = 0; k < EN_NK2; ++k) { const int c = lane + 64 * k; v[k] = c < H2 ? zr[c] : 0.0f; }
        float mean, rstd;
        en_stats<EN_NK2>(v, H2, eps, mean, rstd);
        if (lane == 0) { stats[4 * r + 2] = mean; stats[4 * r + 3] = rstd; }
#pragma unroll
        for (int k = 0; k < EN_NK2; ++k) {
            const int c = lane + 64 * k;
            if (c < H2) zr[c] = act_fwd<1>((v[k] - mean) * rstd * gamma2[c] + beta2[c]);
        }
    }
    __syncthreads();
    en_centre_sums<float>(t, row_ptr, R0, pz, H2, out, ldo);
}

// ================================================================ backward
// part[tile] = (dgamma1 [H1] | dbeta1 [H1] | dgamma2 [H2] | dbeta2 [H2]) of the tile's rows; rows row_ptr[N] .. cap of the three
// edge-row outputs are zeroed (64 per workgroup: gn_linear_wgrad reads all cap rows).
template <typename T>
__global__ __launch_bounds__(256) void edgeconv_norm_bwd_kernel(
    const float* __restrict__ PQ, int H1p, int H1, int H2, const int* __restrict__ row_ptr, const int* __restrict__ jc,
    const int* __restrict__ plan, const T* __restrict__ W2p, const T* __restrict__ W2Tp, const float* __restrict__ b2,
    const float* __restrict__ gamma1, const float* __restrict__ beta1, const float* __restrict__ gamma2,
    const float* __restrict__ beta2, const float* __restrict__ stats, const float* __restrict__ gout, long long ldg,
    int N, long long cap, T* __restrict__ a1g, T* __restrict__ dz2g, T* __restrict__ dpre1g, T* __restrict__ dP, long long lddp,
    float* __restrict__ part, int r0_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char en_lds[];
    __shared__ int cen[EN_ROWS];
    unsigned char* R0 = en_lds;
    unsigned char* WC = en_lds + r0_bytes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int PW = 2 * (H1 + H2);
    {   // rows past the last edge
        const long long E = row_ptr[N];
        const long long lo = E + (long long)blockIdx.x * EN_ROWS, hi = min(lo + EN_ROWS, cap);
        for (long long r = lo + wave; r < hi; r += 4) {
            for (int c = lane; c < H1p; c += 64) { a1g[r * H1p + c] = from_f32<T>(0.0f); dpre1g[r * H1p + c] = from_f32<T>(0.0f); }
            for (int c = lane; c < H2; c += 64) dz2g[r * H2 + c] = from_f32<T>(0.0f);
        }
    }
    const ENTile t = en_tile(plan, row_ptr, cen);
    if (t.c1 <= t.c0) {
        for (int c = threadIdx.x; c < PW; c += 256) part[(long long)blockIdx.x * PW + c] = 0.0f;
        return;
    }
    const int pa = ENCfg<T>::pitch_t(H1p), pz = ENCfg<T>::pitch_f(H2), pd = ENCfg<T>::pitch_t(H2), pg = ENCfg<T>::pitch_f(H1p);
    unsigned char* D = R0 + ENCfg<T>::off_d(H2);

    // ---- pre1 -> a1 -> z2 with the saved statistics
    en_rows_a1<T, false>(t, cen, PQ, H1p, H1, jc, gamma1, beta1, 0.0f, const_cast<float*>(stats), R0, pa, a1g);
    {
        f32x16 acc[2][2];
        en_gemm<T, 2, EN_MAXH2>(R0, pa, W2p, H1p, H2, H1p / BK, WC, acc);
        en_acc_store<2>(acc, H2 / 32, b2, R0, pz);
    }
    // ---- dz2 = LN2' (gelu' (y2) * gout[centre])   (rownorm_act_bwd_kernel's expressions)
    float sdy2[EN_NK2], sdyx2[EN_NK2];
#pragma unroll
    for (int k = 0; k < EN_NK2; ++k) { sdy2[k] = 0.0f; sdyx2[k] = 0.0f; }
    for (int it = 0; it < EN_ROWS / 4; ++it) {
        const int lr = wave * (EN_ROWS / 4) + it;
        if (lr >= t.nr) break;
        const long long r = (long long)t.r0 + lr;
        const float* zr = reinterpret_cast<const float*>(R0 + lr * pz);
        const float* gr = gout + (long long)cen[lr] * ldg;
        const float mean = stats[4 * r + 2], rstd = stats[4 * r + 3];
        float xh[EN_NK2], dy[EN_NK2];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < EN_NK2; ++k) {
            const int c = lane + 64 * k;
            xh[k] = 0.0f; dy[k] = 0.0f;
            if (c < H2) {
                xh[k] = (zr[c] - mean) * rstd;
                const float y = xh[k] * gamma2[c] + beta2[c];
                dy[k] = gr[c] * act_grad<1>(y);
                const float dxh = dy[k] * gamma2[c];
                s1 += dxh;
                s2 += dxh * xh[k];
            }
        }
        s1 = wave_sum(s1) / (float)H2; s2 = wave_sum(s2) / (float)H2;
#pragma unroll
        for (int k = 0; k < EN_NK2; ++k) {
            const int c = lane + 64 * k;
            if (c < H2) {
                const T o = from_f32<T>(rstd * (dy[k] * gamma2[c] - s1 - xh[k] * s2));
                *reinterpret_cast<T*>(D + lr * pd + c * (int)sizeof(T)) = o;
                dz2g[r * H2 + c] = o;
            }
            sdy2[k] += dy[k]; sdyx2[k] += dy[k] * xh[k];
        }
    }
    for (int lr = t.nr + wave; lr < EN_ROWS; lr += 4)
        for (int c = lane; c < H2; c += 64) *reinterpret_cast<T*>(D + lr * pd + c * (int)sizeof(T)) = from_f32<T>(0.0f);
    // ---- da1 = dz2 . W2
    {
        f32x16 acc[2][3];
        en_gemm<T, 3, EN_MAXH1P>(D, pd, W2Tp, H2, H1p, H2 / BK, WC, acc);
        en_acc_store<3>(acc, H1p / 32, nullptr, R0, pg);
    }
    // ---- dpre1 = LN1' (gelu' (y1) * da1), in place in the fp32 tile
    float sdy1[EN_NK1], sdyx1[EN_NK1];
#pragma unroll
    for (int k = 0; k < EN_NK1; ++k) { sdy1[k] = 0.0f; sdyx1[k] = 0.0f; }
    {
        float p[EN_NK1], v[EN_NK1];
        int prev_i = -1;
        for (int it = 0; it < EN_ROWS / 4; ++it) {
            const int lr = wave * (EN_ROWS / 4) + it;
            if (lr >= t.nr) break;
            const long long r = (long long)t.r0 + lr;
            en_gather(PQ, H1p, H1, cen[lr], jc[r], prev_i, p, v);
            float* dr = reinterpret_cast<float*>(R0 + lr * pg);
            const float mean = stats[4 * r], rstd = stats[4 * r + 1];
            float dy[EN_NK1];
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < EN_NK1; ++k) {
                const int c = lane + 64 * k;
                dy[k] = 0.0f;
                if (c < H1) {
                    v[k] = (v[k] - mean) * rstd;                                 // xhat
                    const float y = v[k] * gamma1[c] + beta1[c];
                    dy[k] = dr[c] * act_grad<1>(y);
                    const float dxh = dy[k] * gamma1[c];
                    s1 += dxh;
                    s2 += dxh * v[k];
                }
            }
            s1 = wave_sum(s1) / (float)H1; s2 = wave_sum(s2) / (float)H1;
#pragma unroll
            for (int k = 0; k < EN_NK1; ++k) {
                const int c = lane + 64 * k;
                if (c < H1p) {
                    float o = 0.0f;
                    if (c < H1) o = rstd * (dy[k] * gamma1[c] - s1 - v[k] * s2);
                    dr[c] = o;
                    dpre1g[r * H1p + c] = from_f32<T>(o);
                }
                sdy1[k] += dy[k]; sdyx1[k] += dy[k] * v[k];
            }
        }
    }
    __syncthreads();
    en_centre_sums<T>(t, row_ptr, R0, pg, H1p, dP, lddp);
    // ---- LayerNorm-gradient partials of the tile: the four waves' sums through the (idle) chunk buffer, fixed order
    float* red = reinterpret_cast<float*>(WC);                                   // [4][2][Hmax]
    float* prow = part + (long long)blockIdx.x * PW;
    const int HM = max(H1, H2);
#pragma unroll
    for (int k = 0; k < EN_NK2; ++k) {
        const int c = lane + 64 * k;
        if (c < H2) { red[(wave * 2) * HM + c] = sdyx2[k]; red[(wave * 2 + 1) * HM + c] = sdy2[k]; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H2; c += 256) {
        prow[2 * H1 + c] = (red[0 * HM + c] + red[2 * HM + c]) + (red[4 * HM + c] + red[6 * HM + c]);
        prow[2 * H1 + H2 + c] = (red[1 * HM + c] + red[3 * HM + c]) + (red[5 * HM + c] + red[7 * HM + c]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EN_NK1; ++k) {
        const int c = lane + 64 * k;
        if (c < H1) { red[(wave * 2) * HM + c] = sdyx1[k]; red[(wave * 2 + 1) * HM + c] = sdy1[k]; }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < H1; c += 256) {
        prow[c] = (red[0 * HM + c] + red[2 * HM + c]) + (red[4 * HM + c] + red[6 * HM + c]);
        prow[H1 + c] = (red[1 * HM + c] + red[3 * HM + c]) + (red[5 * HM + c] + red[7 * HM + c]);
    }
}

// ================================================================ launchers
hipError_t launch_edgeconv_norm_plan(const int* row_ptr, int N, int K, int* plan, hipStream_t st) {
    const int ntiles = edgeconv_norm_tiles(N, K);
    if (ntiles < 1 || !row_ptr || !plan) return hipErrorInvalidValue;
    hipLaunchKernelGGL(edgeconv_norm_plan_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, row_ptr, N, EN_ROWS - K,
                       ntiles, plan);
    return hipGetLastError();
}

template <typename K>
static hipError_t en_allow_lds(K kernel, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

template <typename T>
static hipError_t en_fwd(const float* PQ, int H1p, int H1, int H2, const int* row_ptr, const int* jc, const int* plan, int ntiles,
                         const void* W2p, const float* b2, const float* g1, const float* be1, const float* g2, const float* be2,
                         float eps, float* out, long long ldo, float* stats, hipStream_t st) {
    const int r0 = ENCfg<T>::r0_fwd(H1p, H2), lds = r0 + ENCfg<T>::wc(H2);
    static const hipError_t once = en_allow_lds(&edgeconv_norm_fwd_kernel<T>, ENCfg<T>::r0_fwd(EN_MAXH1P, EN_MAXH2) + ENCfg<T>::wc(EN_MAXH2));
    if (once != hipSuccess) return once;
    hipLaunchKernelGGL((edgeconv_norm_fwd_kernel<T>), dim3((unsigned)ntiles), dim3(256), lds, st, PQ, H1p, H1, H2, row_ptr, jc, plan,
                       (const T*)W2p, b2, g1, be1, g2, be2, eps, out, ldo, stats, r0);
    return hipGetLastError();
}
hipError_t launch_edgeconv_norm_fwd(int mode, const float* PQ, int H1p, int H1, int H2, const int* row_ptr, const int* jc,
                                    const int* plan, int ntiles, const void* W2p, const float* b2, const float* g1, const float* be1,
                                    const float* g2, const float* be2, float eps, float* out, long long ldo, float* stats,
                                    hipStream_t st) {
    if (!edgeconv_norm_supported(mode, H1, H2) || H1p != (H1 + 31) / 32 * 32 || ntiles < 1 || ldo < H2) return hipErrorInvalidValue;
    return mode == 1 ? en_fwd<__bf16>(PQ, H1p, H1, H2, row_ptr, jc, plan, ntiles, W2p, b2, g1, be1, g2, be2, eps, out, ldo, stats, st)
                     : en_fwd<float>(PQ, H1p, H1, H2, row_ptr, jc, plan, ntiles, W2p, b2, g1, be1, g2, be2, eps, out, ldo, stats, st);
}

template <typename T>
static hipError_t en_bwd(const float* PQ, int H1p, int H1, int H2, const int* row_ptr, const int* jc, const int* plan, int ntiles,
                         const void* W2p, const void* W2Tp, const float* b2, const float* g1, const float* be1, const float* g2,
                         const float* be2, const float* stats, const float* gout, long long ldg, int N, long long cap, void* a1,
                         void* dz2, void* dpre1, void* dP, long long lddp, float* part, hipStream_t st) {
    const int r0 = ENCfg<T>::r0_bwd(H1p, H2), lds = r0 + ENCfg<T>::wc(max(H1p, H2));
    static const hipError_t once = en_allow_lds(&edgeconv_norm_bwd_kernel<T>, ENCfg<T>::r0_bwd(EN_MAXH1P, EN_MAXH2) + ENCfg<T>::wc(EN_MAXH1P));
    if (once != hipSuccess) return once;
    hipLaunchKernelGGL((edgeconv_norm_bwd_kernel<T>), dim3((unsigned)ntiles), dim3(256), lds, st, PQ, H1p, H1, H2, row_ptr, jc, plan,
                       (const T*)W2p, (const T*)W2Tp, b2, g1, be1, g2, be2, stats, gout, ldg, N, cap, (T*)a1, (T*)dz2, (T*)dpre1,
                       (T*)dP, lddp, part, r0);
    return hipGetLastError();
}
hipError_t launch_edgeconv_norm_bwd(int mode, const float* PQ, int H1p, int H1, int H2, const int* row_ptr, const int* jc,
                                    const int* plan, int ntiles, const void* W2p, const void* W2Tp, const float* b2, const float* g1,
                                    const float* be1, const float* g2, const float* be2, const float* stats, const float* gout,
                                    long long ldg, int N, long long cap, void* a1, void* dz2, void* dpre1, void* dP, long long lddp,
                                    float* part, hipStream_t st) {
    if (!edgeconv_norm_supported(mode, H1, H2) || H1p != (H1 + 31) / 32 * 32 || ntiles < 1 || ldg < H2 || lddp < H1p || N < 0 ||
        cap > (long long)ntiles * EN_ROWS)
        return hipErrorInvalidValue;
    return mode == 1 ? en_bwd<__bf16>(PQ, H1p, H1, H2, row_ptr, jc, plan, ntiles, W2p, W2Tp, b2, g1, be1, g2, be2, stats, gout, ldg, N,
                                      cap, a1, dz2, dpre1, dP, lddp, part, st)
                     : en_bwd<float>(PQ, H1p, H1, H2, row_ptr, jc, plan, ntiles, W2p, W2Tp, b2, g1, be1, g2, be2, stats, gout, ldg, N,
                                     cap, a1, dz2, dpre1, dP, lddp, part, st);
}

}  // namespace gn
