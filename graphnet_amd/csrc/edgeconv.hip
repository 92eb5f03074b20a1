// graphnet_amd/csrc/edgeconv.hip — fused EdgeConv (aggr = add) forward / backward.
//
// Reference op (models/components/layers.py:55-60 -> torch_geometric.nn.EdgeConv):
//     out[i] = sum_{(j->i)} act( W2 . act( W1 . [x_i || x_j - x_i] + b1 ) + b2 )
// Algebraic split used here (SURVEY.md §7 "algebraic shortcut"; rounding differs from the
// reference formulation only in the first linear map, checked at 1e-4 in fp32 mode):
//     W1 . [x_i || x_j - x_i] + b1 = P[i] + Q[j],  P = x (W1a - W1b)^T + b1,  Q = x W1b^T
// P|Q is one per-node GEMM (gemm.hip); this file holds the per-edge part:
//
//   edge_fwd    h = relu(P[i]+Q[j]) built on the fly into the LDS A-tile (gather, never in HBM)
//               -> MFMA with W2 -> +b2, relu -> segmented sum over each centre's slots
//               (in-register + one cross-half shuffle, no atomics) -> out[N,H2];
//               also stores 1 bit per (edge row, column) of the second relu for backward.
//   edge_bwd    dm = g_out[i] (.) bit -> MFMA with W2^T -> (.) [P[i]+Q[j] > 0] = dpre
//               -> segmented slot sum -> dP[i]; dpre rows go to HBM once for the dQ scatter.
//   edge_dw2    dW2 += dm^T . h over all edge rows (contraction over rows; split + slabs),
//               db2 partials.
//   dq_gather   dQ[j] = sum of dpre rows that gathered from j, in ascending row order
//               (reverse adjacency, deterministic).
//
// This file: the generic tiled kernels (any width, fp32 mode, overflow rows) and the dQ gather; the
// persistent operand-stationary bf16 kernels for the table rows of the usual shapes are in edgeconv_v2.hip.
// out / g_out / dP / dQ are stored in the compute type T (fp32 or bf16, see include/graphnet_amd.h).
//
// Edge rows: fixed-stride neighbour table nbr[N,K] (-1 padded) viewed as N*S rows, S = slots
// per centre (8/16/32 >= K); the rare (K+1)-th neighbour of the k+1-then-mask semantics is an
// "overflow" row t (centre ovf_centre[t], source ovf_src[t]) processed by the OVF variants.
#include "launchers.hpp"
#include "edge_v2.hpp"
#include <cstdlib>

namespace gn {

constexpr int EBM = 128;   // edge rows per workgroup tile
constexpr int EBN = 128;   // output columns per workgroup tile


// decode edge row -> (centre, source); source = -1 for empty slots / out of range
// relu, or leaky relu with torch's default slope (DynEdgeJINST)
__device__ __forceinline__ float act01(float x, bool leaky) { return leaky ? fmaxf(x, 0.01f * x) : fmaxf(x, 0.0f); }

template <int S, bool OVF>
__device__ __forceinline__ void row_decode(const EdgeGraph& g, long long row, int& ic, int& jc) {
    ic = 0; jc = -1;
    if constexpr (OVF) {
        if (row < *g.ovf_cnt) { ic = g.ovf_centre[row]; jc = g.ovf_src[row]; }
    } else {
        const long long i = row / S;
        const int s = (int)(row % S);
        if (i < g.N) {
            ic = (int)i;
            if (s < g.K) jc = g.nbr[i * g.K + s];
        }
    }
}

// ------------------------------------------------------------------------------ forward
template <typename T, int S, bool OVF>
__global__ __launch_bounds__(256, 3) void edge_fwd_kernel(
    EdgeGraph g, const T* __restrict__ PQ, int H1p,            // PQ: [N, 2*H1p], P then Q
    const T* __restrict__ W2p, const float* __restrict__ b2, int H2,   // W2p: [H2pad128][H1p]
    T* __restrict__ out, long long ldo,                        // [N, H2] in the compute type (+= for OVF)
    float* __restrict__ coords, CoordCols cc,                  // optional fp32 copy of a few columns
    unsigned int* __restrict__ maskbits,                       // [rows][H2w], H2w = ceil(H2/32)
    bool leaky)                                                // leaky relu (slope 0.01) instead of relu, both activations
{
    constexpr int ROWB = TileCfg<T>::ROWB;
    constexpr int BCHROW = BK * (int)sizeof(T) / 16;
    constexpr int BCH = EBN * BCHROW / 256;
    __shared__ __attribute__((aligned(16))) unsigned char As[EBM * ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[EBN * ROWB];
    __shared__ int s_ic[EBM], s_jc[EBM];

    const long long row0 = (long long)blockIdx.x * EBM;
    if constexpr (OVF) { if (row0 >= *g.ovf_cnt) return; }
    const int n0 = blockIdx.y * EBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int H2w = (H2 + 31) >> 5;
    const long long ldpq = 2LL * H1p;

    if (tid < EBM) {
        int ic, jc;
        row_decode<S, OVF>(g, row0 + tid, ic, jc);
        s_ic[tid] = ic; s_jc[tid] = jc;
    }
    __syncthreads();

    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    int ic[4], jc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ic[i] = s_ic[r0 + 32 * i]; jc[i] = s_jc[r0 + 32 * i]; }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) zero_acc(acc[i][j]);

    f32x4 hreg[4];
    u32x4 breg[BCH];
    const unsigned char* wbytes = reinterpret_cast<const unsigned char*>(W2p);
#define GN_EF_LOAD(kb)                                                                                    \
    {                                                                                                     \
        const int kc = (kb) * BK + c4;                                                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
            f32x4 h = {0.f, 0.f, 0.f, 0.f};                                                               \
            if (jc[i] >= 0) {                                                                             \
                const float4 p = load4<T>(PQ + (long long)ic[i] * ldpq + kc);                             \
                const float4 q = load4<T>(PQ + (long long)jc[i] * ldpq + H1p + kc);                       \
                h[0] = act01(p.x + q.x, leaky); h[1] = act01(p.y + q.y, leaky);                           \
                h[2] = act01(p.z + q.z, leaky); h[3] = act01(p.w + q.w, leaky);                           \
            }                                                                                             \
            hreg[i] = h;                                                                                  \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < BCH; ++i) {                                                 \
            const int ch = tid + 256 * i;                                                                 \
            breg[i] = *reinterpret_cast<const u32x4*>(                                                    \
                wbytes + ((long long)(n0 + ch / BCHROW) * H1p + (kb) * BK) * sizeof(T) + (ch % BCHROW) * 16); \
        }                                                                                                 \
    }

    const int nkb = H1p / BK;
    GN_EF_LOAD(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
            store4<T>(As + (r0 + 32 * i) * ROWB + c4 * sizeof(T), hreg[i][0], hreg[i][1], hreg[i][2], hreg[i][3]);
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
            const int ch = tid + 256 * i;
            *reinterpret_cast<u32x4*>(Bs + (ch / BCHROW) * ROWB + (ch % BCHROW) * 16) = breg[i];
        }
        __syncthreads();
        if (kb + 1 < nkb) GN_EF_LOAD(kb + 1);
        mma_block<T, 2, 2>(As, Bs, wr * 64, wc * 64, lane, acc);
    }
#undef GN_EF_LOAD

    // ---- epilogue: +b2, relu, validity, relu bits, slot sum
    const int h = lane >> 5, cl = lane & 31;
    const int rL = (cl & 3) + 4 * (cl >> 3), hL = (cl >> 2) & 1;   // (reg, half) holding row cl
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
        const int rbase = wr * 64 + tm * 32;                        // first local row of this 32x32 tile
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = n0 + wc * 64 + tn * 32 + cl;
            const bool colok = col < H2;
            const float b = colok ? b2[col] : 0.0f;
            float v[16];
            unsigned int word = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = rbase + acc_row(r, h);
                const bool ok = colok && s_jc[rl] >= 0;
                v[r] = ok ? act01(acc[tm][tn][r] + b, leaky) : 0.0f;          // (leaky(x) > 0 exactly when x > 0)
                const unsigned long long bal = __ballot(v[r] > 0.0f);
                if (r == rL) word = hL ? (unsigned int)(bal >> 32) : (unsigned int)bal;
            }
            if (lane < 32) {
                const long long rowglob = (OVF ? (long long)g.N * S : 0LL) + row0 + rbase + cl;
                const int cw = (n0 + wc * 64 + tn * 32) >> 5;
                const bool rowok = OVF ? (row0 + rbase + cl < *g.ovf_cnt) : (row0 + rbase + cl < (long long)g.N * S);
                if (rowok && cw < H2w) maskbits[rowglob * H2w + cw] = word;
            }
            if constexpr (OVF) {
                // out[centre] += the overflow row's message (at most one overflow row per centre): the old values of the 16
                // rows are requested together, before the first store (written load - add - store per row, every load
                // waited for the store before it)
                float oldv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rbase + acc_row(r, h);
                    oldv[r] = (colok && s_jc[rl] >= 0) ? to_f32(out[(long long)s_ic[rl] * ldo + col]) : 0.0f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rbase + acc_row(r, h);
                    if (colok && s_jc[rl] >= 0) {
                        out[(long long)s_ic[rl] * ldo + col] = from_f32<T>(oldv[r] + v[r]);
                        coord_store(coords, cc, s_ic[rl], col, v[r], true);
                    }
                }
            } else {
                constexpr int CPT = 32 / S;          // centres per 32-row tile
                constexpr int RPC = 16 / CPT;        // accumulator registers per centre per lane
                const long long c0 = (row0 + rbase) / S;
#pragma unroll
                for (int c = 0; c < CPT; ++c) {
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < RPC; ++q) s += v[c * RPC + q];
                    s += __shfl_xor(s, 32);
                    const bool mine = (CPT == 1) ? (h == 0) : ((c * 2 / CPT) == h);
                    if (mine && colok && c0 + c < g.N) {
                        out[(c0 + c) * ldo + col] = from_f32<T>(s);
                        coord_store(coords, cc, c0 + c, col, s, false);
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------ backward (dh)
template <typename T, int S, bool OVF>
__global__ __launch_bounds__(256, 3) void edge_bwd_kernel(
    EdgeGraph g, const T* __restrict__ PQ, int H1p, int H2,
    const T* __restrict__ gout, long long ldg,                 // [N, >=H2] gradient of conv output (compute type)
    const unsigned int* __restrict__ maskbits,
    const T* __restrict__ W2Tp,                                // [H1pad128][H2p] (W2 transposed, packed)
    int H2p,                                                   // H2 padded to 32
    T* __restrict__ dpre,                                      // [rows][H1p]
    T* __restrict__ dP, long long ldp,                         // [N, H1p] in the compute type (= / += for OVF)
    bool leaky)
{
    constexpr int ROWB = TileCfg<T>::ROWB;
    constexpr int BCHROW = BK * (int)sizeof(T) / 16;
    constexpr int BCH = EBN * BCHROW / 256;
    __shared__ __attribute__((aligned(16))) unsigned char As[EBM * ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[EBN * ROWB];
    __shared__ int s_ic[EBM], s_jc[EBM];

    const long long row0 = (long long)blockIdx.x * EBM;
    if constexpr (OVF) { if (row0 >= *g.ovf_cnt) return; }
    const int n0 = blockIdx.y * EBN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int H2w = (H2 + 31) >> 5;
    const long long ldpq = 2LL * H1p;
    const long long rowbase = (OVF ? (long long)g.N * S : 0LL) + row0;

    if (tid < EBM) {
        int ic, jc;
        row_decode<S, OVF>(g, row0 + tid, ic, jc);
        s_ic[tid] = ic; s_jc[tid] = jc;
    }
    __syncthreads();

    const int c4 = (tid & 7) * 4, r0 = tid >> 3;
    int ic[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { ic[i] = s_ic[r0 + 32 * i]; ok[i] = s_jc[r0 + 32 * i] >= 0; }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) zero_acc(acc[i][j]);

    f32x4 areg[4];
    u32x4 breg[BCH];
    const unsigned char* wbytes = reinterpret_cast<const unsigned char*>(W2Tp);
#define GN_EB_LOAD(kb)                                                                                    \
    {                                                                                                     \
        const int kc = (kb) * BK + c4;                                                                    \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
            f32x4 a = {0.f, 0.f, 0.f, 0.f};                                                               \
            if (ok[i] && kc < H2) {                                                                       \
                const unsigned int w = maskbits[(rowbase + r0 + 32 * i) * H2w + (kb)] >> c4;              \
                const float4 gv = load4<T>(gout + (long long)ic[i] * ldg + kc);                           \
                const float sl = leaky ? 0.01f : 0.f;                                                     \
                a[0] = (w & 1u) ? gv.x : (leaky ? sl * gv.x : 0.f); a[1] = (w & 2u) ? gv.y : (leaky ? sl * gv.y : 0.f); \
                a[2] = (w & 4u) ? gv.z : (leaky ? sl * gv.z : 0.f); a[3] = (w & 8u) ? gv.w : (leaky ? sl * gv.w : 0.f); \
            }                                                                                             \
            areg[i] = a;                                                                                  \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < BCH; ++i) {                                                 \
            const int ch = tid + 256 * i;                                                                 \
            breg[i] = *reinterpret_cast<const u32x4*>(                                                    \
                wbytes + ((long long)(n0 + ch / BCHROW) * H2p + (kb) * BK) * sizeof(T) + (ch % BCHROW) * 16); \
        }                                                                                                 \
    }

    const int nkb = H2p / BK;
    GN_EB_LOAD(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
            store4<T>(As + (r0 + 32 * i) * ROWB + c4 * sizeof(T), areg[i][0], areg[i][1], areg[i][2], areg[i][3]);
#pragma unroll
        for (int i = 0; i < BCH; ++i) {
            const int ch = tid + 256 * i;
            *reinterpret_cast<u32x4*>(Bs + (ch / BCHROW) * ROWB + (ch % BCHROW) * 16) = breg[i];
        }
        __syncthreads();
        if (kb + 1 < nkb) GN_EB_LOAD(kb + 1);
        mma_block<T, 2, 2>(As, Bs, wr * 64, wc * 64, lane, acc);
    }
#undef GN_EB_LOAD

    // [P[i] + Q[j] > 0] of the tile's 128 rows x 128 columns as bits in LDS: two threads per row read its P and Q
    // segments with 16-byte loads (read element by element in the epilogue below - two 2-byte loads per dpre element -
    // this was most of the kernel's time on tie-heavy graphs, where the overflow rows run here by the ten thousand)
    __shared__ unsigned int s_hb[EBM][EBN / 32];
    {
        const int hr = tid >> 1, hc0 = n0 + (tid & 1) * (EBN / 2);
        const int hi_ = s_ic[hr], hj_ = s_jc[hr];
        unsigned int w0 = 0u, w1 = 0u;
        if (hj_ >= 0) {
#pragma unroll
            for (int q = 0; q < EBN / 8; ++q) {
                const int cq = hc0 + 4 * q;
                if (cq < H1p) {                                                  // H1p is a multiple of 32
                    const float4 p = load4<T>(PQ + (long long)hi_ * ldpq + cq);
                    const float4 qv = load4<T>(PQ + (long long)hj_ * ldpq + H1p + cq);
                    const unsigned int b4 = (p.x + qv.x > 0.0f ? 1u : 0u) | (p.y + qv.y > 0.0f ? 2u : 0u) |
                                            (p.z + qv.z > 0.0f ? 4u : 0u) | (p.w + qv.w > 0.0f ? 8u : 0u);
                    if (q < 8) w0 |= b4 << (4 * q); else w1 |= b4 << (4 * (q - 8));
                }
            }
        }
        s_hb[hr][(tid & 1) * 2] = w0;
        s_hb[hr][(tid & 1) * 2 + 1] = w1;
    }
    __syncthreads();
    const int h = lane >> 5, cl = lane & 31;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
        const int rbase = wr * 64 + tm * 32;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = n0 + wc * 64 + tn * 32 + cl;
            const bool colok = col < H1p;
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rl = rbase + acc_row(r, h);
                const int j = s_jc[rl];
                float d = 0.0f;
                if (colok && j >= 0) {
                    const bool pos = (s_hb[rl][wc * 2 + tn] >> cl) & 1u;
                    d = pos ? acc[tm][tn][r] : (leaky ? 0.01f * acc[tm][tn][r] : 0.0f);
                }
                v[r] = d;
                const long long rg = row0 + rl;
                const bool rowok = OVF ? (rg < *g.ovf_cnt) : (rg < (long long)g.N * S);
                if (colok && rowok) dpre[(rowbase + rl) * H1p + col] = from_f32<T>(d);
            }
            if constexpr (OVF) {
                float oldv[16];                          // (loads first, then the stores: see edge_fwd_kernel)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rbase + acc_row(r, h);
                    oldv[r] = (colok && s_jc[rl] >= 0) ? to_f32(dP[(long long)s_ic[rl] * ldp + col]) : 0.0f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rl = rbase + acc_row(r, h);
                    if (colok && s_jc[rl] >= 0) dP[(long long)s_ic[rl] * ldp + col] = from_f32<T>(oldv[r] + v[r]);
                }
            } else {
                constexpr int CPT = 32 / S, RPC = 16 / CPT;
                const long long c0 = (row0 + rbase) / S;
#pragma unroll
                for (int c = 0; c < CPT; ++c) {
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < RPC; ++q) s += v[c * RPC + q];
                    s += __shfl_xor(s, 32);
                    const bool mine = (CPT == 1) ? (h == 0) : ((c * 2 / CPT) == h);
                    if (mine && colok && c0 + c < g.N) dP[(c0 + c) * ldp + col] = from_f32<T>(s);
                }
            }
        }
    }
}

// rows per split of the overflow-row dW2 launch for cnt overflow rows (multiple of BK = 32, at least one block): shared by
// the kernel and by reduce_slabs2_kernel (gemm.hip), which must count the same non-empty splits
__host__ __device__ __forceinline__ int dw2_ovf_rows_per_split(int cnt, int splits) {
    const int r = (cnt + splits - 1) / splits;
    return r < 1 ? 32 : (r + 31) / 32 * 32;
}
// ------------------------------------------------------------------------------ dW2 / db2
// slab[split][n2][k1] = sum over this split's edge rows of dm[row][n2] * h[row][k1]
// Rows enumerate the table rows [0, N*S) followed by the overflow rows [N*S, N*S + cnt).
template <typename T, int S>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 3 : 2) void edge_dw2_kernel(
    EdgeGraph g, const T* __restrict__ PQ, int H1p, int H1, int H2,
    const T* __restrict__ gout, long long ldg, const unsigned int* __restrict__ maskbits,
    long long row_begin, long long rows_per_split, float* __restrict__ slab, float* __restrict__ db2_part, int n2_tiles,
    bool leaky, bool skip_empty)        // skip_empty: a split > 0 without rows writes nothing (launch_edge_dw2_reduce skips it)
{
    constexpr int ROWB = TileCfg<T>::ROWB;
    constexpr int BT = 128;
    constexpr int RS = ROWB / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) unsigned char As[BT * ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Bs[BT * ROWB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int t2 = blockIdx.x % n2_tiles, tk = blockIdx.x / n2_tiles;
    const int n2_0 = t2 * BT, k1_0 = tk * BT;
    const int split = blockIdx.y;
    const int H2w = (H2 + 31) >> 5;
    const long long ldpq = 2LL * H1p;
    const long long main_rows = (long long)g.N * S;
    const long long total_rows = main_rows + (g.ovf_cnt ? *g.ovf_cnt : 0);
    // skip_empty (the overflow-row launch behind the persistent kernel): the row ranges are cut from the ACTUAL number of
    // overflow rows (device side), not from the N possible ones - a tie-heavy graph (learned coordinates that collapse onto
    // shared values: 20-40k overflow rows at B = 1024 after a few hundred optimizer steps) then spreads over all the
    // splits instead of the first few (264 -> 60 us per launch); a split > 0 without rows writes nothing
    if (skip_empty) rows_per_split = dw2_ovf_rows_per_split((int)(total_rows - main_rows), (int)gridDim.y);
    const long long rbeg = row_begin + split * rows_per_split;
    const long long rend = min(total_rows, rbeg + rows_per_split);
    if (skip_empty && split > 0 && rbeg >= rend) return;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) zero_acc(acc[i][j]);
    float bsum[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bsum[i] = 0.0f;

    const int mr = tid >> 3, cb = (tid & 7) * 4;
    f32x4 ra[4], rb[4];
#define GN_DW_LOAD(rb0)                                                                                   \
    {                                                                                                     \
        const long long row = (rb0) + mr;                                                                 \
        int ic = 0, jc = -1;                                                                              \
        if (row < rend) {                                                                                 \
            if (row < main_rows) row_decode<S, false>(g, row, ic, jc);                                    \
            else { ic = g.ovf_centre[row - main_rows]; jc = g.ovf_src[row - main_rows]; }                 \
        }                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};                                     \
            const int ca = n2_0 + cb + 32 * i;                                                            \
            const int ck = k1_0 + cb + 32 * i;                                                            \
            if (jc >= 0 && ca < H2) {                                                                     \
                const unsigned int w = maskbits[row * H2w + (ca >> 5)] >> (ca & 31);                      \
                const float4 gv = load4<T>(gout + (long long)ic * ldg + ca);                              \
                const float sl = leaky ? 0.01f : 0.f;                                                     \
                a[0] = (w & 1u) ? gv.x : (leaky ? sl * gv.x : 0.f); a[1] = (w & 2u) ? gv.y : (leaky ? sl * gv.y : 0.f); \
                a[2] = (w & 4u) ? gv.z : (leaky ? sl * gv.z : 0.f); a[3] = (w & 8u) ? gv.w : (leaky ? sl * gv.w : 0.f); \
            }                                                                                             \
            if (jc >= 0 && ck < H1p) {                                                                    \
                const float4 p = load4<T>(PQ + (long long)ic * ldpq + ck);                                \
                const float4 q = load4<T>(PQ + (long long)jc * ldpq + H1p + ck);                          \
                b[0] = act01(p.x + q.x, leaky); b[1] = act01(p.y + q.y, leaky);                           \
                b[2] = act01(p.z + q.z, leaky); b[3] = act01(p.w + q.w, leaky);                           \
            }                                                                                             \
            ra[i] = a; rb[i] = b;                                                                         \
        }                                                                                                 \
    }

    if (rbeg < rend) GN_DW_LOAD(rbeg);
    for (long long r0 = rbeg; r0 < rend; r0 += BK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cb + 32 * i;
            T* pa = reinterpret_cast<T*>(As + c * ROWB) + mr;
            T* pb = reinterpret_cast<T*>(Bs + c * ROWB) + mr;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T av = from_f32<T>(ra[i][q]);
                pa[q * RS] = av;
                pb[q * RS] = from_f32<T>(rb[i][q]);
                bsum[i * 4 + q] += ra[i][q];
            }
        }
        __syncthreads();
        if (r0 + BK < rend) GN_DW_LOAD(r0 + BK);
        mma_block<T, 2, 2>(As, Bs, wr * 64, wc * 64, lane, acc);
    }
#undef GN_DW_LOAD

    const int h = lane >> 5, cl = lane & 31;
    const long long Ks = H1;                                  // slab row pitch = real H1
    float* out = slab + (long long)split * H2 * Ks;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kc = k1_0 + wc * 64 + j * 32 + cl;
            if (kc >= H1) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n2 = n2_0 + wr * 64 + i * 32 + acc_row(r, h);
                if (n2 < H2) out[(long long)n2 * Ks + kc] = acc[i][j][r];
            }
        }
    // db2 partial: column sums of dm over this split (only the k1-tile-0 workgroups write it).
    // 32 row-threads x 128 columns are reduced through As in two halves of 16 rows (8 KB).
    if (tk == 0) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(As);
        for (int half = 0; half < 2; ++half) {
            if ((mr >> 4) == half) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int q = 0; q < 4; ++q) red[(mr & 15) * 128 + cb + 32 * i + q] = bsum[i * 4 + q];
            }
            __syncthreads();
            if (tid < 128) {
                float s = 0.0f;
                for (int r = 0; r < 16; ++r) s += red[r * 128 + tid];
                const int n2 = n2_0 + tid;
                if (n2 < H2) {
                    float* dst = db2_part + (long long)split * H2 + n2;
                    *dst = half ? *dst + s : s;
                }
            }
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------ dQ gather
// dQ[j][:] = sum of dpre rows listed in rev_rows[rev_ptr[j]..rev_ptr[j+1]) in ascending row id.
// One wave per source node.  The in-edge list is filled with atomics (arbitrary order), so the wave first
// sorts it (rank by counting, one ds_permute) and then streams the rows in ascending row id with eight
// row loads in flight: fixed summation order -> bitwise reproducible, and enough bytes in flight for HBM.
template <typename T>
__device__ __forceinline__ void dq_row_load(const T* row, int col, bool ok, float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        u32x4 raw = {0u, 0u, 0u, 0u};
        if (ok) raw = *reinterpret_cast<const u32x4*>(row + col);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const unsigned u = raw[w];
            v[2 * w] = __builtin_bit_cast(float, u << 16);
            v[2 * w + 1] = __builtin_bit_cast(float, u & 0xffff0000u);
        }
    } else {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (ok) {
            a = *reinterpret_cast<const float4*>(row + col);
            b = *reinterpret_cast<const float4*>(row + col + 4);
        }
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
}

constexpr int DQ_HUB_MIN = 64, DQ_HUB_CAP = 16384;     // = REV_SORT_MIN / REV_SORT_CAP of graph.hip
template <typename T>
__global__ __launch_bounds__(256) void dq_gather_kernel(const T* __restrict__ dpre, int H1p,
                                                        const int* __restrict__ rev_ptr, const int* __restrict__ rev_rows,
                                                        int N, T* __restrict__ dQ, long long ldq, int skip_hubs) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= N) return;
    const int lo = rev_ptr[j], hi = rev_ptr[j + 1];
    const int deg = hi - lo;
    if (skip_hubs && deg > DQ_HUB_MIN && deg <= DQ_HUB_CAP) return;       // dq_hub_kernel sums this node
    // lane owns columns [8*lane, 8*lane+8) (pass 0) and [512 + 8*lane, ...) is never needed: H1p <= 512
    const int col = lane * 8;
    const bool ok = col < H1p;                                // H1p is a multiple of 8 on this path
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.0f;

    if (deg <= 64) {
        const int r = lane < deg ? rev_rows[lo + lane] : 0x7fffffff;
        int rank = 0;
        for (int t = 0; t < deg; ++t) rank += (__shfl(r, t) < r) ? 1 : 0;      // row ids are distinct
        // lanes >= deg hold INT_MAX: rank = deg (collide harmlessly on slot deg..; keep them out of the way)
        const int slot = lane < deg ? rank : lane;
        const int sorted = __builtin_amdgcn_ds_permute(slot << 2, r);
        int t = 0;
        for (; t + 8 <= deg; t += 8) {
            float v[8][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int row = __shfl(sorted, t + u);
                dq_row_load<T>(dpre + (long long)row * H1p, col, ok, v[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += v[u][c];
        }
        if (t < deg) {
            float v[8][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int row = __shfl(sorted, min(t + u, deg - 1));
                dq_row_load<T>(dpre + (long long)row * H1p, col, ok && (t + u < deg), v[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += v[u][c];       // + 0.0f for the masked rows: exact
        }
    } else if (deg <= 16384) {
        // hub node: its list was sorted by rev_sort_kernel (graph.hip) -> stream it, 8 rows in flight
        int t = 0;
        for (; t + 8 <= deg; t += 8) {
            float v[8][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) dq_row_load<T>(dpre + (long long)rev_rows[lo + t + u] * H1p, col, ok, v[u]);
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += v[u][c];
        }
        for (; t < deg; ++t) {
            float v[8];
            dq_row_load<T>(dpre + (long long)rev_rows[lo + t] * H1p, col, ok, v);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] += v[c];
        }
    } else {
        int last = -1;
        for (int t = lo; t < hi; ++t) {
            // beyond the sort capacity: next row id in ascending order = min over entries > last (O(deg^2/64))
            int best = 0x7fffffff;
            for (int e = lo + lane; e < hi; e += 64) {
                const int r = rev_rows[e];
                if (r > last && r < best) best = r;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
            last = best;
            float v[8];
            dq_row_load<T>(dpre + (long long)best * H1p, col, ok, v);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] += v[c];
        }
    }
    if (ok) {
        T* dst = dQ + (long long)j * ldq + col;
        store4<T>(dst, acc[0], acc[1], acc[2], acc[3]);
        store4<T>(dst + 4, acc[4], acc[5], acc[6], acc[7]);
    }
}

// Hub nodes (sorted in-edge lists of 65..16384 rows): one 16-wave workgroup per hub.  Wave w sums the row
// blocks b = w, w+16, ... (8 rows each, loaded together) in ascending order, the 16 partial sums are added
// in wave order: a fixed order, so the result is reproducible, and 16 x 8 rows are in flight per hub.
constexpr int DQ_HUB_WAVES = 16;
template <typename T>
__global__ __launch_bounds__(DQ_HUB_WAVES * 64) void dq_hub_kernel(const T* __restrict__ dpre, int H1p,
                                                                    const int* __restrict__ rev_ptr,
                                                                    const int* __restrict__ rev_rows,
                                                                    const int* __restrict__ hubs, const int* __restrict__ nhubs,
                                                                    T* __restrict__ dQ, long long ldq) {
    __shared__ float part[DQ_HUB_WAVES][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane * 8;
    const bool ok = col < H1p;
    const int n = *nhubs;
    for (int t = blockIdx.x; t < n; t += gridDim.x) {
        const int j = hubs[t];
        const int lo = rev_ptr[j], deg = rev_ptr[j + 1] - lo;
        float acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.0f;
        for (int b0 = wave * 8; b0 < deg; b0 += DQ_HUB_WAVES * 8) {
            float v[8][8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = min(b0 + u, deg - 1);
                dq_row_load<T>(dpre + (long long)rev_rows[lo + e] * H1p, col, ok && (b0 + u < deg), v[u]);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += v[u][c];
        }
        if (ok) {
#pragma unroll
            for (int c = 0; c < 8; ++c) part[wave][col + c] = acc[c];
        }
        __syncthreads();
        for (int c = threadIdx.x; c < H1p; c += DQ_HUB_WAVES * 64) {
            float s = part[0][c];
#pragma unroll
            for (int w = 1; w < DQ_HUB_WAVES; ++w) s += part[w][c];
            dQ[(long long)j * ldq + c] = from_f32<T>(s);
        }
        __syncthreads();
    }
}

}  // namespace gn

namespace gn {
// ------------------------------------------------------------------------------ overflow rows on the GEMM kernels
// A tie-heavy graph (learned k-NN coordinates that collapse onto shared values) has tens of thousands of overflow rows; the
// tiled kernels above cost ~30x a persistent-kernel row for each.  For the DynEdge shape in bf16 mode (relu) the overflow
// rows are materialised instead - h rows [cnt][H1p], messages m [cnt][H2] (both kept in `saved`) - and run through the
// weights-stationary / transposed-operand GEMM kernels with the row count read on the device (Epi::m_dev):
//   forward   h = relu(P[c] + Q[s])  ->  m = relu(h W2^T + b2)  ->  out[c] += m, coords, slot bits of the rows
//   dW2       dm = g_out[c] (m > 0)  ->  partial slabs dm^T h (+ db2 from the ones block) behind the main parts
//   backward  dpre rows = (dm W2) (h > 0) written in place  ->  dP[c] += row
// (c, s: centre / source of the overflow row; at most one overflow row per centre, so the adds do not collide).
typedef __bf16 bf16x8_e __attribute__((ext_vector_type(8)));
// (leaky variant, DynEdgeJINST: h = leaky(P + Q); the GEMMs then run WITHOUT their relu / gate epilogues and the second
// activation, its slope and the first activation's slope are applied by the scatter / dm kernels below)
__global__ __launch_bounds__(256) void ovf_gather_h_kernel(EdgeGraph g, const __bf16* __restrict__ PQ, int H1p, __bf16* __restrict__ h,
                                                           bool leaky) {
    const int cnt = *g.ovf_cnt, lane = threadIdx.x & 63;
    const int col = lane * 8;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < cnt; t += gridDim.x * 4) {
        if (col >= H1p) continue;
        const long long ldpq = 2LL * H1p;
        const bf16x8_e p = *reinterpret_cast<const bf16x8_e*>(PQ + (long long)g.ovf_centre[t] * ldpq + col);
        const bf16x8_e q = *reinterpret_cast<const bf16x8_e*>(PQ + (long long)g.ovf_src[t] * ldpq + H1p + col);
        bf16x8_e o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)act01((float)p[e] + (float)q[e], leaky);
        *reinterpret_cast<bf16x8_e*>(h + (long long)t * H1p + col) = o;
    }
}
// out[c] += m[t] (bf16, one rounding of the sum), fp32 coordinate copy, and the row's [m > 0] bits into the slot-bit words
// of row N * S + t (what the tiled dW2 / backward kernels read: they stay valid fallbacks)
__global__ __launch_bounds__(256) void ovf_scatter_fwd_kernel(EdgeGraph g, const __bf16* __restrict__ m, int H2, __bf16* __restrict__ out,
                                                              long long ldo, float* __restrict__ coords, CoordCols cc,
                                                              unsigned int* __restrict__ words, int S, bool leaky) {
    const int cnt = *g.ovf_cnt, H2w = H2 >> 5;
    const long long total = (long long)cnt * H2w;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int t = (int)(idx / H2w), w = (int)(idx % H2w);
        const int c = g.ovf_centre[t];
        unsigned int bits = 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 32 * w + 8 * q;
            const bf16x8_e mv = *reinterpret_cast<const bf16x8_e*>(m + (long long)t * H2 + col);
            bf16x8_e* op = reinterpret_cast<bf16x8_e*>(out + (long long)c * ldo + col);
            bf16x8_e ov = *op;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float x = (float)mv[e];                  // relu: m itself; leaky: the pre-activation
                bits |= (x > 0.0f ? 1u : 0u) << (8 * q + e);
                const float v = leaky ? fmaxf(x, 0.01f * x) : x;
                ov[e] = (__bf16)((float)ov[e] + v);
                coord_store(coords, cc, c, col + e, v, true);
            }
            *op = ov;
        }
        words[((long long)g.N * S + t) * H2w + w] = bits;
    }
}
__global__ __launch_bounds__(256) void ovf_dm_kernel(EdgeGraph g, const __bf16* __restrict__ m, int H2, const __bf16* __restrict__ gout,
                                                     long long ldg, __bf16* __restrict__ dm, bool leaky) {
    const int cnt = *g.ovf_cnt, ch = H2 >> 3;
    const long long total = (long long)cnt * ch;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int t = (int)(idx / ch), col = (int)(idx % ch) * 8;
        const bf16x8_e mv = *reinterpret_cast<const bf16x8_e*>(m + (long long)t * H2 + col);
        const bf16x8_e gv = *reinterpret_cast<const bf16x8_e*>(gout + (long long)g.ovf_centre[t] * ldg + col);
        bf16x8_e o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)mv[e] > 0.0f ? gv[e] : (leaky ? (__bf16)(0.01f * (float)gv[e]) : (__bf16)0.0f);
        *reinterpret_cast<bf16x8_e*>(dm + (long long)t * H2 + col) = o;
    }
}
// leaky: the rows arrive as dm W2 (no gate in the GEMM): the first activation's slope (1 where h > 0, 0.01 elsewhere) is
// applied here, in place, before the add
__global__ __launch_bounds__(256) void ovf_scatter_dp_kernel(EdgeGraph g, __bf16* __restrict__ rows, int H1p, __bf16* __restrict__ dP,
                                                             long long ldp, const __bf16* __restrict__ h_leaky) {
    const int cnt = *g.ovf_cnt, ch = H1p >> 3;
    const long long total = (long long)cnt * ch;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int t = (int)(idx / ch), col = (int)(idx % ch) * 8;
        bf16x8_e rv = *reinterpret_cast<const bf16x8_e*>(rows + (long long)t * H1p + col);
        if (h_leaky) {
            const bf16x8_e hv = *reinterpret_cast<const bf16x8_e*>(h_leaky + (long long)t * H1p + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) rv[e] = (float)hv[e] > 0.0f ? rv[e] : (__bf16)(0.01f * (float)rv[e]);
            *reinterpret_cast<bf16x8_e*>(rows + (long long)t * H1p + col) = rv;
        }
        bf16x8_e* dp = reinterpret_cast<bf16x8_e*>(dP + (long long)g.ovf_centre[t] * ldp + col);
        bf16x8_e o = *dp;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)((float)o[e] + (float)rv[e]);
        *dp = o;
    }
}

}  // namespace gn

// =============================================================== host launchers
namespace gn {

static inline int cdiv__(long long a, long long b) { return (int)((a + b - 1) / b); }
int edge_slots(int K) { return K <= 8 ? 8 : (K <= 16 ? 16 : 32); }
long long edge_dw2_splits(long long rows) {
    long long s = (rows + 4095) / 4096;
    if (s < 1) s = 1;
    if (s > 512) s = 512;
    return s;
}

#define GN_DISPATCH_S(S_, CALL)            \
    switch (S_) {                          \
        case 8: { constexpr int S = 8; CALL; } break;   \
        case 16: { constexpr int S = 16; CALL; } break; \
        default: { constexpr int S = 32; CALL; } break; \
    }

constexpr int DW2_OVF_SPLITS = 128;   // x 6 column tiles = 768 workgroups at most (only the splits that hold rows run): tie-heavy graphs have ~N overflow rows

int device_cus() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}

template <typename T>
static hipError_t edge_fwd_t(const EdgeGraph& g, const void* PQ, int H1p, const void* W2p, const float* b2, int H2,
                             void* out, long long ldo, float* coords, const CoordCols& cc, unsigned int* maskbits,
                             bool main_rows, bool leaky, hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    const int S_ = edge_slots(g.K);
    const int ny = cdiv__(H2, EBN);
    GN_DISPATCH_S(S_, {
        if (main_rows)
            hipLaunchKernelGGL((edge_fwd_kernel<T, S, false>), dim3(cdiv__((long long)g.N * S, EBM), ny), dim3(256), 0, st,
                               g, (const T*)PQ, H1p, (const T*)W2p, b2, H2, (T*)out, ldo, coords, cc, maskbits, leaky);
        if (g.ovf_cnt)
            hipLaunchKernelGGL((edge_fwd_kernel<T, S, true>), dim3(cdiv__(g.N, EBM), ny), dim3(256), 0, st,
                               g, (const T*)PQ, H1p, (const T*)W2p, b2, H2, (T*)out, ldo, coords, cc, maskbits, leaky);
    });
    return hipGetLastError();
}
// The environment switches of the edge path (the only reader under csrc/):
//   GN_DISABLE_V2=1          tiled kernels for everything (A/B tests flip it inside one process: read on every call)
//   GN_OVF_GEMM=0            overflow rows stay on the tiled overflow-row kernels instead of the GEMM path (A/B)
//   GN_DPRE_COMPACT=1        the model paths take the compact-dpre kernels.  OPT-IN: exact and bit-identical, but measured
//                            SLOWER than the dense pair at B = 4096 (edge bwd 0.98 -> 1.56 ms per launch: the in-place
//                            halfword scatter is a phase of its own that nothing overlaps; gather 0.75 -> 1.3 ms: two
//                            dependent loads per row and ~50 vector + ~60 scalar instructions per row) - DESIGN.md section 7h
//   GN_EDGE_WS=<mask>        bit 0: wave-specialised relu forward (default 7: on)
//   GN_WS_PRODUCERS_FIRST=n  which waves of the wave-specialised forward gather (round 2: producers on the four oldest
//                            waves -1 %; re-measured at the end of round 3, after the consumer loop had changed: producers on
//                            the YOUNGEST waves -2.2 .. -3.4 % on the forward kernel, two alternating pairs at B = 4096 -
//                            default 0 now)
// All but the first are read once per process.
EdgeSwitches edge_switches() {
    static const EdgeSwitches once = [] {
        EdgeSwitches s = {};
        const char* e = getenv("GN_OVF_GEMM"); s.ovf_gemm = !(e && e[0] == '0');
        e = getenv("GN_DPRE_COMPACT"); s.dpre_compact = e && e[0] == '1';
        e = getenv("GN_EDGE_WS"); s.edge_ws = e ? atoi(e) : 7;
        e = getenv("GN_WS_PRODUCERS_FIRST"); s.producers_first = e ? atoi(e) : 0;
        return s;
    }();
    EdgeSwitches s = once;
    const char* e = getenv("GN_DISABLE_V2");
    s.disable_v2 = e && e[0] == '1';
    return s;
}
// The plan of a layer (edge_plan.hpp).  Forward, dW2, its reduction and the backward call this with the same arguments, so
// they agree on what `saved` holds; act: 0 = relu after both layers (DynEdge), 1 = leaky relu + max aggregation
// (EdgeConvTito, models/components/layers.py:72-114), 2 = leaky relu after both layers + add (DynEdgeJINST, models/gnn/
// dynedge_jinst.py:56-98).
static EdgePlan plan_of(int mode, const EdgeGraph& g, int H1p, int H1, int H2, int act) {
    return edge_plan(mode, g.K, g.N, H1p, H1, H2, act, g.ovf_cnt != nullptr, edge_switches());
}
static const unsigned long long* tilevalid_of(const EdgePlan& p, const unsigned char* sb, const SavedLayout& L) {
    return p.variant == 2 ? reinterpret_cast<const unsigned long long*>(sb + L.off_valid) : nullptr;
}
// ---- overflow rows on the GEMM kernels (kernels above), EdgePlan::ovf == 2
static int ovf_grid(long long work_items) {
    const long long b = (work_items + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
static Segs ovf_seg(const void* p, long long ld, int width) {
    Segs s;
    s.nseg = 1; s.p[0] = p; s.ld[0] = ld; s.width[0] = width; s.kpad[0] = (width + 31) / 32 * 32;
    return s;
}
static hipError_t launch_ovf_fwd(const EdgeGraph& g, const void* PQ, int H1p, const void* W2p, const float* b2, int H2, void* out,
                                 long long ldo, float* coords, const CoordCols& cc, unsigned char* sb, const SavedLayout& L,
                                 hipStream_t st, bool leaky) {
    __bf16* h = reinterpret_cast<__bf16*>(sb + L.off_ovf_h);
    __bf16* m = reinterpret_cast<__bf16*>(sb + L.off_ovf_m);
    hipLaunchKernelGGL(ovf_gather_h_kernel, dim3(ovf_grid((long long)g.N * 64)), dim3(256), 0, st, g, (const __bf16*)PQ, H1p, h, leaky);
    Epi e;
    e.bias = b2; e.gate = nullptr; e.ldgate = 0; e.relu = leaky ? 0 : 1; e.accum = 0; e.gate_lowp = 0; e.m_dev = g.ovf_cnt;
    hipError_t r = launch_gemm_nt(1, ovf_seg(h, H1p, H1p), 1, g.N, W2p, H1p, (H2 + 127) / 128 * 128, H2, e, m, H2, 1, st);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(ovf_scatter_fwd_kernel, dim3(ovf_grid((long long)g.N * (H2 / 32))), dim3(256), 0, st, g, (const __bf16*)m, H2,
                       (__bf16*)out, ldo, coords, cc, reinterpret_cast<unsigned int*>(sb + L.off_words), edge_slots(g.K), leaky);
    return hipGetLastError();
}
// dpre rows of the overflow rows = (dm W2) (h > 0) -> rows [cnt][H1p]; dP[c] += row.  dm: left in `saved` by launch_edge_dw2
static hipError_t launch_ovf_bwd(const EdgeGraph& g, int H1p, int H2, const unsigned char* sb, const SavedLayout& L, const void* W2Tp,
                                 int H2p, __bf16* rows, void* dP, long long ldp, hipStream_t st, bool leaky) {
    const __bf16* h = reinterpret_cast<const __bf16*>(sb + L.off_ovf_h);
    const __bf16* dm = reinterpret_cast<const __bf16*>(sb + L.off_ovf_dm);
    Epi e;
    e.bias = nullptr; e.gate = leaky ? nullptr : h; e.ldgate = leaky ? 0 : H1p; e.relu = 0; e.accum = 0; e.gate_lowp = leaky ? 0 : 1;
    e.m_dev = g.ovf_cnt;
    hipError_t r = launch_gemm_nt(1, ovf_seg(dm, H2, H2), 1, g.N, W2Tp, H2p, (H1p + 127) / 128 * 128, H1p, e, rows, H1p, 1, st);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(ovf_scatter_dp_kernel, dim3(ovf_grid((long long)g.N * (H1p / 8))), dim3(256), 0, st, g, rows, H1p,
                       (__bf16*)dP, ldp, leaky ? h : (const __bf16*)nullptr);
    return hipGetLastError();
}
int edge_leaky_supported(int mode, int K, int H1p, int H1, int H2) {
    return edge_plan(mode, K, 0, H1p, H1, H2, 2, false, edge_switches()).persistent;
}
int edge_max_supported(int mode, int K, int H1p, int H2) {
    return edge_plan(mode, K, 0, H1p, H1p, H2, 1, false, edge_switches()).supported;
}
// The plan of a layer as the launchers below take it, under this process's switches (host only: tests name the path they
// mean to run and skip a shape outside a path's envelope by this answer).  out[8] = supported, persistent, variant, ovf,
// compact_shape, compact_model, shape_persistent, and whether the persistent forward is the wave-specialised kernel
// (`out` rows of pitch H2)
void edge_plan_query(int mode, int K, long long N, int H1p, int H1, int H2, int act, bool has_ovf, int* out) {
    const EdgeSwitches sw = edge_switches();
    const EdgePlan p = edge_plan(mode, K, N, H1p, H1, H2, act, has_ovf, sw);
    EdgeGraph g = {};
    g.N = (int)N; g.K = K;
    out[0] = p.supported; out[1] = p.persistent; out[2] = p.variant; out[3] = p.ovf;
    out[4] = p.compact_shape; out[5] = p.compact_model; out[6] = p.shape_persistent;
    out[7] = p.persistent && edge_fwd_v2_ws(p.variant, g, H1p, H1, H2, H2, sw);
}

// out is float in mode 0 and bf16 in mode 1; coords (optional, [N][8] fp32) receives the columns
// coord_cols[0..ncoord) of the fp32 result (the next layer's k-NN coordinates).
// act = 1 (EdgeConvTito): fused kernels for bf16 tables WITHOUT overflow rows, K <= 16, H1p = H2 = 256 only -
// hipErrorNotSupported otherwise (all three passes): the caller then runs the unfused edge-row path (csrc/generic.hip).
hipError_t launch_edge_fwd(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H1, const void* W2p, const float* b2,
                           int H2, void* out, long long ldo, float* coords, const int* coord_cols, int ncoord,
                           void* saved, hipStream_t st, int act) {
    const EdgePlan p = plan_of(mode, g, H1p, H1, H2, act);
    if (act < 0 || act > 2) return hipErrorInvalidValue;
    if (!p.supported) return hipErrorNotSupported;
    if (H1p % BK || g.K > 32 || ncoord < 0 || ncoord > 8) return hipErrorInvalidValue;
    const bool leaky = p.variant == 2;
    CoordCols cc;
    cc.n = coords ? ncoord : 0;
    for (int d = 0; d < 8; ++d) cc.c[d] = (d < cc.n) ? coord_cols[d] : -1;
    if (cc.n == 0) coords = nullptr;
    const SavedLayout L = saved_layout(g.N, edge_slots(g.K), H1p, H2);
    unsigned char* sb = reinterpret_cast<unsigned char*>(saved);
    unsigned int* words = reinterpret_cast<unsigned int*>(sb + L.off_words);
    if (mode == 0) return edge_fwd_t<float>(g, PQ, H1p, W2p, b2, H2, out, ldo, coords, cc, words, true, leaky, st);
    // bf16: persistent weights-stationary kernel for the table rows when the shape allows it
    if (p.persistent) {
        hipError_t e = launch_edge_fwd_v2(p.variant, g, PQ, H1p, H1, W2p, b2, H2, out, ldo, coords, cc, sb + L.off_maskB,
                                          const_cast<unsigned long long*>(tilevalid_of(p, sb, L)), device_cus(), st);
        if (e != hipSuccess) return e;
    }
    if (p.ovf == 2) return launch_ovf_fwd(g, PQ, H1p, W2p, b2, H2, out, ldo, coords, cc, sb, L, st, leaky);
    return edge_fwd_t<__bf16>(g, PQ, H1p, W2p, b2, H2, out, ldo, coords, cc, words, !p.persistent, leaky, st);
}

template <typename T>
static hipError_t edge_bwd_t(const EdgeGraph& g, const void* PQ, int H1p, int H2, const void* gout, long long ldg,
                             const unsigned int* maskbits, const void* W2Tp, int H2p, void* dpre, void* dP,
                             long long ldp, bool main_rows, bool leaky, hipStream_t st) {
    if (g.N == 0) return hipSuccess;
    const int S_ = edge_slots(g.K);
    const int ny = cdiv__(H1p, EBN);
    GN_DISPATCH_S(S_, {
        if (main_rows)
            hipLaunchKernelGGL((edge_bwd_kernel<T, S, false>), dim3(cdiv__((long long)g.N * S, EBM), ny), dim3(256), 0, st,
                               g, (const T*)PQ, H1p, H2, (const T*)gout, ldg, maskbits, (const T*)W2Tp, H2p, (T*)dpre,
                               (T*)dP, ldp, leaky);
        if (g.ovf_cnt)
            hipLaunchKernelGGL((edge_bwd_kernel<T, S, true>), dim3(cdiv__(g.N, EBM), ny), dim3(256), 0, st,
                               g, (const T*)PQ, H1p, H2, (const T*)gout, ldg, maskbits, (const T*)W2Tp, H2p, (T*)dpre,
                               (T*)dP, ldp, leaky);
    });
    return hipGetLastError();
}
// gout and dP are float in mode 0 and bf16 in mode 1.  H1: as given to the forward with act 1 / 2 (not needed with act 0)
hipError_t launch_edge_bwd(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H2, const void* gout,
                           long long ldg, const void* saved, const void* W2Tp, int H2p, void* dpre,
                           void* dP, long long ldp, hipStream_t st, int act, int H1) {
    const EdgePlan p = plan_of(mode, g, H1p, H1, H2, act);
    if (act < 0 || act > 2) return hipErrorInvalidValue;
    if (!p.supported) return hipErrorNotSupported;
    if (H1p % BK || H2p % BK || g.K > 32 || (ldg & (mode ? 7 : 3)) || (ldp & (mode ? 7 : 3))) return hipErrorInvalidValue;
    const bool leaky = p.variant == 2;
    const SavedLayout L = saved_layout(g.N, edge_slots(g.K), H1p, H2);
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(saved);
    const unsigned int* words = reinterpret_cast<const unsigned int*>(sb + L.off_words);
    if (mode == 0) return edge_bwd_t<float>(g, PQ, H1p, H2, gout, ldg, words, W2Tp, H2p, dpre, dP, ldp, true, leaky, st);
    if (p.persistent) {      // needs hbits: launch_edge_dw2 of this layer must have run before; H2p == 256 or not supported
        hipError_t e = launch_edge_bwd_v2(p.variant, g, H1p, H2, gout, ldg, sb + L.off_maskB, sb + L.off_hbits, tilevalid_of(p, sb, L),
                                          W2Tp, H2p, dpre, dP, ldp, device_cus(), st);
        if (e != hipSuccess) return e;
    }
    if (p.ovf == 2)
        return launch_ovf_bwd(g, H1p, H2, sb, L, W2Tp, H2p, reinterpret_cast<__bf16*>(dpre) + (long long)g.N * edge_slots(g.K) * H1p,
                              dP, ldp, st, leaky);
    return edge_bwd_t<__bf16>(g, PQ, H1p, H2, gout, ldg, words, W2Tp, H2p, dpre, dP, ldp, !p.persistent, leaky, st);
}

// ---- compact dpre (csrc/dpre_compact.hip): plan workspace = [rowoff u16 tiles*64 | tilesize16 int tiles | tilebase int tiles |
// scan tmp], all 256-byte aligned
static inline long long up256(long long v) { return (v + 255) / 256 * 256; }
DprePlan dpre_plan_layout(int N, int K, void* base) {
    const long long tiles = dpre_compact_tiles(N, K) > 0 ? dpre_compact_tiles(N, K) : 1;
    unsigned char* b = reinterpret_cast<unsigned char*>(base);
    DprePlan p;
    long long off = 0;
    p.rowoff = reinterpret_cast<unsigned short*>(b + off); off += up256(tiles * 64 * 2);
    p.tilesize16 = reinterpret_cast<int*>(b + off); off += up256(tiles * 4);
    p.tilebase = reinterpret_cast<int*>(b + off); off += up256(tiles * 4);
    p.tmp = reinterpret_cast<int*>(b + off); off += up256(((tiles + 2047) / 2048 + 2) * 4);
    p.total = off;
    return p;
}
// whether the MODEL paths (step entry, per-op backward) choose the compact kernels (EdgePlan::compact_model; the explicit
// entry points run whenever the shape allows, EdgePlan::compact_shape)
int dpre_compact_supported(int mode, int K, int H1p, int H1, int H2) {
    return edge_plan(mode, K, 0, H1p, H1, H2, 0, false, edge_switches()).compact_model;
}
long long dpre_compact_bytes(int N, int K, int H1p) { return dpre_compact_tiles(N, K) * 64 * H1p * 2 + 256; }
hipError_t launch_dpre_plan_saved(int N, int K, int H1p, int H1, int H2, const void* saved, void* plan, hipStream_t st) {
    const SavedLayout L = saved_layout(N, edge_slots(K), H1p, H2);
    const DprePlan p = dpre_plan_layout(N, K, plan);
    return launch_dpre_plan(N, K, H1p, H1, reinterpret_cast<const unsigned char*>(saved) + L.off_hbits, p.rowoff, p.tilesize16,
                            p.tilebase, p.tmp, st);
}
// table rows -> compact stream dpre_c; overflow rows -> dense rows dpre_ovf[t][H1p] (t = overflow row index)
hipError_t launch_edge_bwd_cp(const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout, long long ldg,
                              const void* saved, const void* W2Tp, int H2p, void* plan, void* dpre_c, void* dpre_ovf, void* dP,
                              long long ldp, hipStream_t st) {
    const EdgePlan pl = plan_of(1, g, H1p, H1, H2, 0);
    if (!pl.compact_shape) return hipErrorNotSupported;
    if (H1p % BK || H2p % BK || (ldg & 7) || (ldp & 7)) return hipErrorInvalidValue;
    const int S_ = edge_slots(g.K);
    const SavedLayout L = saved_layout(g.N, S_, H1p, H2);
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(saved);
    const DprePlan p = dpre_plan_layout(g.N, g.K, plan);
    BwdCompact cp;
    cp.rowoff = p.rowoff; cp.tilebase = p.tilebase; cp.tilesize16 = p.tilesize16;
    cp.dpre_c = reinterpret_cast<unsigned char*>(dpre_c); cp.creal = (H1 + 7) / 8;
    hipError_t e = launch_edge_bwd_v2(0, g, H1p, H2, gout, ldg, sb + L.off_maskB, sb + L.off_hbits, nullptr, W2Tp, H2p, nullptr, dP,
                                      ldp, device_cus(), st, &cp);
    if (e != hipSuccess) return e;
    if (dpre_ovf && pl.ovf == 2)                                        // same overflow-row path as the dense pair
        return launch_ovf_bwd(g, H1p, H2, sb, L, W2Tp, H2p, reinterpret_cast<__bf16*>(dpre_ovf), dP, ldp, st, false);
    // the generic kernel addresses overflow row t as row N * S + t of ONE dpre array: hand it that array's virtual base
    __bf16* virt = dpre_ovf ? reinterpret_cast<__bf16*>(dpre_ovf) - (long long)g.N * S_ * H1p : nullptr;
    return edge_bwd_t<__bf16>(g, PQ, H1p, H2, gout, ldg, reinterpret_cast<const unsigned int*>(sb + L.off_words), W2Tp, H2p, virt, dP,
                              ldp, false, false, st);
}
hipError_t launch_dq_gather_cp_saved(int N, int K, int H1p, int H1, int H2, const void* saved, const void* plan, const void* dpre_c,
                                     const void* dpre_ovf, const int* rev_ptr, const int* rev_rows, const int* hubs,
                                     const int* nhubs, void* dQ, long long ldq, hipStream_t st) {
    if ((ldq & 7)) return hipErrorInvalidValue;
    const SavedLayout L = saved_layout(N, edge_slots(K), H1p, H2);
    const DprePlan p = dpre_plan_layout(N, K, const_cast<void*>(plan));
    return launch_dq_gather_cp(N, K, H1p, H1, reinterpret_cast<const unsigned char*>(dpre_c), p.tilebase, p.rowoff,
                               reinterpret_cast<const unsigned char*>(saved) + L.off_hbits, dpre_ovf, rev_ptr, rev_rows, hubs, nhubs,
                               dQ, ldq, st);
}

// Partial results: slab[nslab][H2][H1], db2_part[nslab][H2] with nslab = edge_dw2_slabs(); the caller
// reduces them in fixed order (launch_reduce_slabs in gemm.hip).
// parts of the transposed-operand GEMM that takes the overflow rows' dW2 (0: not applicable - the tiled kernel does it)
static int ovf_dw2_gemm_parts(int N, int H1, int H2) {
    if ((H1 & 7) || (H2 & 7)) return 0;
    const int p = gemm_tn_parts(1, N, H2, &H1, 1);
    return p <= DW2_OVF_SPLITS ? p : 0;
}
// The slab accounting of one layer's dW2.  total: what the caller allocates (edge_dw2_slabs) - the count of the SHAPE,
// whatever the activation or the overflow list: outside the persistent envelope of the leaky variant the tiled kernel
// spreads the rows over all of them.  The first nmain are always written; of the next novf, as many as `rps` says
// (launch_reduce_slabs2: 1 = plain slabs, 0 = cut from the device-side overflow count, -1 = the GEMM's parts, all written).
struct Dw2Slabs { int total, nmain, novf, rps; };
static Dw2Slabs dw2_slabs(const EdgePlan& p, int N, int K, int H1p, int H1, int H2, int cus) {
    Dw2Slabs s;
    const int parts = edge_dw2_v2_parts(N, K, H1p, cus);
    s.total = !p.shape_persistent ? (int)edge_dw2_splits((long long)N * edge_slots(K) + N)
                                  : parts + (p.variant == 1 ? 0 : DW2_OVF_SPLITS);       // act 1: never overflow rows
    s.nmain = s.total; s.novf = 0; s.rps = 1;
    if (p.persistent) {
        const int gemm_parts = p.ovf == 2 ? ovf_dw2_gemm_parts(N, H1, H2) : 0;
        s.nmain = parts;
        s.novf = gemm_parts > 0 ? gemm_parts : (p.ovf ? DW2_OVF_SPLITS : 0);
        s.rps = gemm_parts > 0 ? -1 : 0;
    }
    return s;
}
int edge_dw2_slabs(int mode, int N, int K, int H1p, int H2) {
    return dw2_slabs(edge_plan(mode, K, N, H1p, H1p, H2, 0, false, edge_switches()), N, K, H1p, H1p, H2, device_cus()).total;
}
int edge_max_dw2_slabs(int N, int K, int H1p) { return edge_dw2_v2_parts(N, K, H1p, device_cus()); }   // act 1: no overflow rows

static long long dw2_rows_per_split(long long rows, int splits) {
    const long long rps = (rows + splits - 1) / splits;
    return (rps + BK - 1) / BK * BK;
}
template <typename T>
static hipError_t edge_dw2_t(const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout,
                             long long ldg, const unsigned int* maskbits, long long row_begin, long long rows,
                             float* slab, float* db2_part, int splits, bool leaky, hipStream_t st, bool skip_empty = false) {
    const int S_ = edge_slots(g.K);
    const long long rps = dw2_rows_per_split(rows, splits);
    const int n2t = cdiv__(H2, 128), kt = cdiv__(H1, 128);
    GN_DISPATCH_S(S_, {
        hipLaunchKernelGGL((edge_dw2_kernel<T, S>), dim3(n2t * kt, splits), dim3(256), 0, st,
                           g, (const T*)PQ, H1p, H1, H2, (const T*)gout, ldg, maskbits, row_begin, rps, slab, db2_part, n2t, leaky, skip_empty);
    });
    return hipGetLastError();
}
hipError_t launch_edge_dw2(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout,
                           long long ldg, void* saved, float* slab, float* db2_part, hipStream_t st, int act) {
    const EdgePlan p = plan_of(mode, g, H1p, H1, H2, act);
    if (act < 0 || act > 2) return hipErrorInvalidValue;
    if (!p.supported) return hipErrorNotSupported;
    if (g.N == 0 || (ldg & (mode ? 7 : 3))) return hipErrorInvalidValue;
    const Dw2Slabs s = dw2_slabs(p, g.N, g.K, H1p, H1, H2, device_cus());
    const bool leaky = p.variant == 2;
    const int S_ = edge_slots(g.K);
    const SavedLayout L = saved_layout(g.N, S_, H1p, H2);
    unsigned char* sb = reinterpret_cast<unsigned char*>(saved);
    const unsigned int* words = reinterpret_cast<const unsigned int*>(sb + L.off_words);
    const long long main_rows = (long long)g.N * S_;
    if (mode == 0) return edge_dw2_t<float>(g, PQ, H1p, H1, H2, gout, ldg, words, 0, main_rows + g.N, slab, db2_part, s.total, leaky, st);
    if (!p.persistent)
        return edge_dw2_t<__bf16>(g, PQ, H1p, H1, H2, gout, ldg, words, 0, main_rows + g.N, slab, db2_part, s.total, leaky, st);
    // persistent kernel for the table rows (also writes hbits), then the overflow rows behind its s.nmain parts
    hipError_t e = launch_edge_dw2_v2(p.variant, g, PQ, H1p, H1, H2, gout, ldg, sb + L.off_maskB, sb + L.off_hbits,
                                      tilevalid_of(p, sb, L), slab, db2_part, device_cus(), st);
    if (e != hipSuccess) return e;
    if (!p.ovf) return hipSuccess;
    float* ovf_slab = slab + (long long)s.nmain * H2 * H1;
    float* ovf_db2 = db2_part + (long long)s.nmain * H2;
    if (p.ovf == 2) {
        // dm = g_out[c] (m > 0) (also the backward's operand), then - real hidden width a multiple of 8 - the partial slabs
        // dm^T h from the transposed-operand GEMM
        const __bf16* h = reinterpret_cast<const __bf16*>(sb + L.off_ovf_h);
        const __bf16* m = reinterpret_cast<const __bf16*>(sb + L.off_ovf_m);
        __bf16* dm = reinterpret_cast<__bf16*>(sb + L.off_ovf_dm);
        hipLaunchKernelGGL(ovf_dm_kernel, dim3(ovf_grid((long long)g.N * (H2 / 8))), dim3(256), 0, st, g, m, H2, (const __bf16*)gout, ldg, dm,
                           leaky);
        if (s.rps == -1) return launch_gemm_tn_parts_only(dm, H2, H2, h, H1p, H1, g.N, g.ovf_cnt, ovf_slab, ovf_db2, st);
    }
    // tiled kernel: DW2_OVF_SPLITS row ranges over the N possible ones; a range without rows writes nothing (except the
    // first): with a handful of overflow rows 39 of the 40 slabs were zeros written here and read back by the reduction
    return edge_dw2_t<__bf16>(g, PQ, H1p, H1, H2, gout, ldg, words, main_rows, g.N, ovf_slab, ovf_db2, DW2_OVF_SPLITS, leaky, st, true);
}
hipError_t launch_edge_dw2_reduce(int mode, const EdgeGraph& g, int H1p, int H1, int H2, const float* slab, const float* db2_part,
                                  float* dW2, float* db2, hipStream_t st, int act) {
    if (g.N == 0) return hipErrorInvalidValue;
    const Dw2Slabs s = dw2_slabs(plan_of(mode, g, H1p, H1, H2, act), g.N, g.K, H1p, H1, H2, device_cus());
    return launch_reduce_slabs2(slab, (long long)H2 * H1, dW2, db2_part, H2, db2, s.nmain, s.novf, g.ovf_cnt, s.rps, st);
}

// dQ is float in mode 0 and bf16 in mode 1 (like dpre)
// hubs / nhubs (optional): the hub list rev_build left behind; those nodes are then summed by 16 waves each
hipError_t launch_dq_gather(int mode, const void* dpre, int H1p, const int* rev_ptr, const int* rev_rows,
                            const int* hubs, const int* nhubs, int N, void* dQ, long long ldq, hipStream_t st) {
    if (N == 0) return hipSuccess;
    if (H1p > 512 || (H1p & 7) || (ldq & (mode ? 7 : 3))) return hipErrorInvalidValue;
    const int skip = (hubs && nhubs) ? 1 : 0;
    const dim3 hgrid(256), hblock(DQ_HUB_WAVES * 64);
    if (mode == 0) {
        hipLaunchKernelGGL((dq_gather_kernel<float>), dim3(cdiv__(N, 4)), dim3(256), 0, st, (const float*)dpre, H1p,
                           rev_ptr, rev_rows, N, (float*)dQ, ldq, skip);
        if (skip)
            hipLaunchKernelGGL((dq_hub_kernel<float>), hgrid, hblock, 0, st, (const float*)dpre, H1p, rev_ptr, rev_rows,
                               hubs, nhubs, (float*)dQ, ldq);
    } else {
        hipLaunchKernelGGL((dq_gather_kernel<__bf16>), dim3(cdiv__(N, 4)), dim3(256), 0, st, (const __bf16*)dpre, H1p,
                           rev_ptr, rev_rows, N, (__bf16*)dQ, ldq, skip);
        if (skip)
            hipLaunchKernelGGL((dq_hub_kernel<__bf16>), hgrid, hblock, 0, st, (const __bf16*)dpre, H1p, rev_ptr, rev_rows,
                               hubs, nhubs, (__bf16*)dQ, ldq);
    }
    return hipGetLastError();
}

}  // namespace gn
