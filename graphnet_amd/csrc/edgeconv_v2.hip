// graphnet_amd/csrc/edgeconv_v2.hip — persistent, operand-stationary fused EdgeConv kernels (bf16).
//
// MI355X-specific structure (512-entry unified VGPR file, 160 KB LDS, 256 CUs):
//   * one 512-thread workgroup (8 waves, 2 per SIMD) per CU, persistent over a CONTIGUOUS range of
//     64-row edge tiles (8 centres x 8 slots): an event's tiles stay on one CU, so the Q rows it
//     gathers (each reused by ~K centres) are L1/L2 hits;
//   * the small operand of each contraction never moves: edge_fwd_v2 keeps its W2 slice (K x 32
//     per wave) in registers as MFMA B fragments, edge_bwd_v2 its W2^T slices, edge_dw2_v2 keeps
//     the whole dW2 accumulator (256 x H1p fp32 = 176 VGPRs per lane) in registers;
//   * the gathered operand (h = relu(P[i]+Q[j]) or dm = g_out[i] (.) relu-bits) is built
//     cooperatively into double-buffered LDS tiles while the MFMAs of the previous tile run
//     (issue-early / write-late, branch-free, one barrier per tile);
//   * dW2 contracts over edge rows: its h^T fragments come from the row-major LDS tile through
//     ds_read_b64_tr_b16 (hardware transpose), its dm^T fragments are built in registers from one
//     g_out value + one "slot byte" per lane and k-step (the 8 rows of a k-step half are the 8
//     slots of ONE centre).
//
// Saved-for-backward formats (region offsets: saved_layout() in common.hpp):
//   maskB[centre][H2]  uint8, bit s = second-relu active for slot s     (written by edge_fwd_v2)
//   hbits[row][H1p/8]  uint8, bit c%8 of byte c/8 = h[row][c] > 0        (written by edge_dw2_v2)
//
// Envelope: bf16, K <= 16 (S = 8 or 16 slots), H1p in {128, 352} (256 for the max variant), H2 == 256: the shape tests are
// in edge_plan.hpp.  Anything else, the overflow rows, and f32 mode run the generic kernels of edgeconv.hip.
#include "edge_v2.hpp"

namespace gn {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int V2_ROWS = 64;     // edge rows per tile = 64 / S centres x S slots (S = 8 or 16 slots per centre)
constexpr int V2_THREADS = 512;

__device__ __forceinline__ unsigned int pack_bf16x2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));   // one v_cvt_pk_bf16_f32
}

// fp32 adds in this file stay PLAIN v_add_f32: the Makefile builds it with -fno-slp-vectorize.  Left to itself the
// compiler pairs adjacent scalar adds into v_pk_add_f32, and beside MFMAs a packed-f32 instruction costs more issue
// time than the two it replaces (MI355X guide, "packed f32 VALU ... an anti-lever beside MFMAs"; here: forward
// 1.237 -> 1.17 ms per launch).  (Inline-asm adds are not an option for MFMA results: the hazard recognizer does not
// see an asm statement's reads, and the epilogue then read accumulators the MFMA had not written yet.)
__device__ __forceinline__ void add2_f32(float a0, float b0, float a1, float b1, float& s0, float& s1) {
    s0 = a0 + b0;
    s1 = a1 + b1;
}
// relu(p + q) on 8 packed bf16: unpack with shift/and, f32 adds, one cvt_pk per pair, relu as a
// packed signed-16-bit max with 0 (bf16 is sign-magnitude: negative <=> int16 < 0).
__device__ __forceinline__ u32x4 relu_sum_bf16x8(u32x4 p, u32x4 q) {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float plo = __builtin_bit_cast(float, p[w] << 16), phi = __builtin_bit_cast(float, p[w] & 0xffff0000u);
        const float qlo = __builtin_bit_cast(float, q[w] << 16), qhi = __builtin_bit_cast(float, q[w] & 0xffff0000u);
        float slo, shi;
        add2_f32(plo, qlo, phi, qhi, slo, shi);
        const unsigned int s = pack_bf16x2(slo, shi);
        const s16x2 m = __builtin_elementwise_max(__builtin_bit_cast(s16x2, s), (s16x2){0, 0});
        o[w] = __builtin_bit_cast(unsigned int, m);
    }
    return o;
}
// EdgeConvTito variant (models/components/layers.py:72-114: LeakyReLU edge MLP, max aggregation): h = leaky_relu(p + q)
// = max(x, 0.01 x) in fp32 before the rounding to bf16 (torch's default negative_slope)
__device__ __forceinline__ u32x4 leaky_sum_bf16x8(u32x4 p, u32x4 q) {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const float plo = __builtin_bit_cast(float, p[w] << 16), phi = __builtin_bit_cast(float, p[w] & 0xffff0000u);
        const float qlo = __builtin_bit_cast(float, q[w] << 16), qhi = __builtin_bit_cast(float, q[w] & 0xffff0000u);
        float xl, xh;
        add2_f32(plo, qlo, phi, qhi, xl, xh);
        o[w] = pack_bf16x2(fmaxf(xl, 0.01f * xl), fmaxf(xh, 0.01f * xh));
    }
    return o;
}
// V = 0: relu (DynEdge), V = 1: leaky relu + max aggregation (EdgeConvTito), V = 2: leaky relu + add aggregation with a
// leaky relu after the second layer too (DynEdgeJINST, models/gnn/dynedge_jinst.py:56-98)
template <int V> __device__ __forceinline__ u32x4 act_sum_bf16x8(u32x4 p, u32x4 q) {
    if constexpr (V == 0) return relu_sum_bf16x8(p, q);
    else return leaky_sum_bf16x8(p, q);
}
// 8 "h > 0" flags of a packed bf16x8 that may hold NEGATIVE values (leaky relu): as signed 16-bit integers a bf16 is
// > 0 exactly when its integer is > 0 (sign-magnitude, -0.0 = 0x8000 < 0): clamp to [0, 1], then as below
__device__ __forceinline__ unsigned int positive_bits_bf16x8(u32x4 o) {
    unsigned int t = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned int ow = o[w];                    // copy the element first: bit_cast of a vector-element lvalue reads element 0
        const s16x2 c = __builtin_elementwise_min(__builtin_elementwise_max(__builtin_bit_cast(s16x2, ow), (s16x2){0, 0}),
                                                  (s16x2){1, 1});
        const unsigned int k = (1u << (2 * w)) | (2u << (2 * w + 16));
        t = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, c), __builtin_bit_cast(u16x2, k), t, false);
    }
    return t;
}
// 8 "h > 0" flags of a packed NON-NEGATIVE bf16x8 (bit c = column c of the chunk): min(half, 1) is the flag of a
// half in [0, 0x7fff]; a 16-bit dot product with the weights (2^2w, 2^(2w+1)) drops both flags of a dword into place:
// two instructions per dword.
__device__ __forceinline__ unsigned int nonzero_bits_bf16x8(u32x4 o) {
    unsigned int t = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        unsigned int y;
        asm("v_pk_min_u16 %0, %1, %2" : "=v"(y) : "v"(o[w]), "s"(0x00010001u));       // the compiler expands the builtin min
        const unsigned int c = (1u << (2 * w)) | (2u << (2 * w + 16));
        t = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, y), __builtin_bit_cast(u16x2, c), t, false);
    }
    return t;
}

// ---- shared gather machinery (8 threads per row, thread handles 16-byte chunks (tid&7)+8i) --------
// Branch-free: out-of-range rows/chunks are clamped to valid addresses (duplicate chunks write
// identical bytes).  Row info is fetched in two halves so that its load is issued FIRST in an
// iteration and consumed LAST (vmcnt is in-order: an early use would drain the whole gather).
#define GN_V2_INFO_ISSUE(tile_, ic_, raw_, ok_)                                                       \
    {                                                                                                 \
        long long row__ = (long long)(tile_) * V2_ROWS + grow;                                        \
        const bool inr__ = ((tile_) < ntiles) && (row__ < main_rows);                                 \
        row__ = inr__ ? row__ : 0;                                                                    \
        const int ii__ = (int)(row__ / S), sl__ = (int)(row__ % S);        /* S: power of two */      \
        const int slc__ = sl__ < kslots ? sl__ : 0;                                                   \
        (raw_) = g.nbr[(long long)ii__ * kslots + slc__];                                             \
        (ic_) = ii__;                                                                                 \
        (ok_) = inr__ && sl__ < kslots;                                                               \
    }
#define GN_V2_INFO(tile_, ic_, jc_)                                                                   \
    {                                                                                                 \
        int raw__; bool ok__;                                                                         \
        GN_V2_INFO_ISSUE(tile_, ic_, raw__, ok__);                                                    \
        (jc_) = ok__ ? raw__ : -1;                                                                    \
    }
// gathers chunks cbeg_ + (tid&7) + 8i, i < NI_, clamped to cend_-1, of P[ic] and Q[jc]
#define GN_V2_GATHER_WIN(ic_, jc_, cbeg_, cend_, NI_)                                                 \
    {                                                                                                 \
        const int js__ = (jc_) < 0 ? 0 : (jc_);                                                       \
        const __bf16* pp__ = PQ + (long long)(ic_) * ldpq;                                            \
        const __bf16* qq__ = PQ + (long long)js__ * ldpq + K;                                         \
        _Pragma("unroll") for (int i = 0; i < (NI_); ++i) {                                           \
            const int c__ = (cbeg_) + gc0 + 8 * i;                                                    \
            const int cc__ = c__ < (cend_) ? c__ : (cend_) - 1;                                       \
            preg[i] = *reinterpret_cast<const u32x4*>(pp__ + cc__ * 8);                               \
            qreg[i] = *reinterpret_cast<const u32x4*>(qq__ + cc__ * 8);                               \
        }                                                                                             \
    }

// =============================================================================== forward
// S = slots per centre (8 or 16); the slot mask of (centre, column) is S bits: maskB is uint8 / uint16 [N][H2].
template <int KSTEPS, int S>
__global__ __launch_bounds__(V2_THREADS, 2) void edge_fwd_v2_kernel(
    EdgeGraph g, const __bf16* __restrict__ PQ, const __bf16* __restrict__ W2p, const float* __restrict__ b2,
    int H2, __bf16* __restrict__ out, long long ldo, float* __restrict__ coords, CoordCols ccols,
    unsigned char* __restrict__ maskB, int ntiles)
{
    static_assert(S == 8 || S == 16, "8 or 16 slots per centre");
    constexpr int NST = 16 / S;                    // centres stored per lane and 32-row block: 2 (S=8) / 1 (S=16)
    constexpr int K = KSTEPS * 16;                 // = H1p
    constexpr int ROWB = K * 2 + 16;               // LDS row pitch: conflict-free ds_read_b128
    constexpr int CHUNKS = K / 8;
    __shared__ __attribute__((aligned(16))) unsigned char As[2][V2_ROWS * ROWB];
    __shared__ int s_jc[2][V2_ROWS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long ldpq = 2LL * K;
    const long long main_rows = (long long)g.N * S;
    const bool wave_on = wave * 32 < H2;
    const int kslots = g.K;

    bf16x8 w2[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) w2[s][e] = (__bf16)0.0f;
    if (wave_on) {
        const __bf16* wrow = W2p + (long long)(wave * 32 + r) * K + h * 8;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) w2[s] = *reinterpret_cast<const bf16x8*>(wrow + s * 16);
    }
    const int col = wave * 32 + r;
    const float bias = (col < H2) ? b2[col] : 0.0f;
    // does this lane's column feed the fp32 coordinate copy (next layer's k-NN)?
    int coord_d = -1;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if (coords && d < ccols.n && ccols.c[d] == col) coord_d = d;
    const bool is_coord = coord_d >= 0;

    // the gather of a tile is split in two chunk windows (registers: 2 x 3 x 16 B in flight)
    constexpr int CH_A = (CHUNKS / 2 + 7) / 8 * 8 < CHUNKS ? (CHUNKS / 2 + 7) / 8 * 8 : CHUNKS;   // first window
    constexpr int NI_A = CH_A / 8, NI_B = (CHUNKS - CH_A + 7) / 8;
    constexpr int NI = NI_A > NI_B ? NI_A : NI_B;
    const int grow = tid >> 3, gc0 = tid & 7;
    u32x4 preg[NI > 0 ? NI : 1], qreg[NI > 0 ? NI : 1];
#define GN_V2_WRITE_H(buf_, cbeg_, cend_, NI_)                                                        \
    {                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < (NI_); ++i) {                                           \
            const int c__ = (cbeg_) + gc0 + 8 * i;                                                    \
            const int cc__ = c__ < (cend_) ? c__ : (cend_) - 1;                                       \
            *reinterpret_cast<u32x4*>(&As[buf_][grow * ROWB + cc__ * 16]) = relu_sum_bf16x8(preg[i], qreg[i]); \
        }                                                                                             \
    }

    const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    int tile = blockIdx.x * per;
    const int tile_end = min(ntiles, tile + per);
    int ic_n, jc_n;
    {
        int ic, jc;
        GN_V2_INFO(tile, ic, jc);
        GN_V2_GATHER_WIN(ic, jc, 0, CH_A, NI_A);
        GN_V2_WRITE_H(0, 0, CH_A, NI_A);
        if (NI_B > 0) {
            GN_V2_GATHER_WIN(ic, jc, CH_A, CHUNKS, NI_B);
            GN_V2_WRITE_H(0, CH_A, CHUNKS, NI_B);
        }
        if (gc0 == 0) s_jc[0][grow] = jc;
        GN_V2_INFO(tile + 1, ic_n, jc_n);
    }
    __syncthreads();

    int buf = 0;
    for (; tile < tile_end; ++tile, buf ^= 1) {
        int ic_nn, raw_nn;
        bool ok_nn;
        GN_V2_INFO_ISSUE(tile + 2, ic_nn, raw_nn, ok_nn);
        GN_V2_GATHER_WIN(ic_n, jc_n, 0, CH_A, NI_A);

        f32x16 acc0, acc1;
#pragma unroll
        for (int q = 0; q < 16; ++q) { acc0[q] = bias; acc1[q] = bias; }
        float st_sum[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
        unsigned int st_msk = 0;                    // S=8: 4 bytes (rb, c2); S=16: 2 halfwords (rb)
        if (wave_on) {
            const unsigned char* a0 = &As[buf][r * ROWB + h * 16];
            const unsigned char* a1 = a0 + 32 * ROWB;
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                const bf16x8 f0 = *reinterpret_cast<const bf16x8*>(a0 + s * 32);
                const bf16x8 f1 = *reinterpret_cast<const bf16x8*>(a1 + s * 32);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0, w2[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, w2[s], acc1, 0, 0, 0);
                if (s == KSTEPS / 2 - 1 && NI_B > 0) {      // mid-tile: retire window A, issue window B
                    GN_V2_WRITE_H(buf ^ 1, 0, CH_A, NI_A);
                    GN_V2_GATHER_WIN(ic_n, jc_n, CH_A, CHUNKS, NI_B);
                }
            }

            // ---- epilogue: relu, slot bytes (sign trick, no ballots), slot sums
            const unsigned long long vbits = __ballot(s_jc[buf][lane] >= 0);     // bit = tile row
            const bool all_valid = (vbits == ~0ull);                              // wave-uniform
            const unsigned int vrow0 = (unsigned int)(vbits >> (4 * h));          // row block 0, this half
            const unsigned int vrow1 = (unsigned int)(vbits >> (32 + 4 * h));     // row block 1
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                const f32x16& acc = rb ? acc1 : acc0;
                float sums[4];
                unsigned int pack = 0;
#pragma unroll
                for (int c = 3; c >= 0; --c) {
                    float sum = 0.0f;
                    unsigned int nib = 0;
                    if (all_valid) {            // wave-uniform: almost every tile; no per-element selects
#pragma unroll
                        for (int qq = 3; qq >= 0; --qq) {
                            const float x = acc[4 * c + qq];
                            sum += fmaxf(x, 0.0f);
                            const float y = 0.0f - x;                             // sign(y) = [x > 0]
                            nib = __builtin_amdgcn_alignbit(nib, __builtin_bit_cast(unsigned int, y), 31);
                        }
                    } else {
#pragma unroll
                        for (int qq = 3; qq >= 0; --qq) {
                            const int q = 4 * c + qq;
                            const float x = (((rb ? vrow1 : vrow0) >> acc_row(q, 0)) & 1u) ? acc[q] : -1.0f;
                            sum += fmaxf(x, 0.0f);
                            const float y = 0.0f - x;
                            nib = __builtin_amdgcn_alignbit(nib, __builtin_bit_cast(unsigned int, y), 31);
                        }
                    }
                    sums[c] = sum;
                    pack = (pack << 4) | nib;
                }
                const unsigned int other = __shfl_xor(pack, 32);
                const unsigned int lo16 = h ? other : pack, hi16 = h ? pack : other;   // slots 0-3 / 4-7
                if constexpr (S == 8) {
                    // this lane stores centres c = 2h, 2h+1 of the row block (stores issued at the end of the iteration)
#pragma unroll
                    for (int cc = 0; cc < 2; ++cc) {
                        const float mine = h ? sums[2 + cc] : sums[cc];
                        const float theirs = h ? sums[cc] : sums[2 + cc];          // what the partner lane needs
                        st_sum[rb][cc] = mine + __shfl_xor(theirs, 32);
                        const int sh = 4 * (2 * h + cc);
                        st_msk |= (((lo16 >> sh) & 0xFu) | (((hi16 >> sh) & 0xFu) << 4)) << (8 * (2 * rb + cc));
                    }
                } else {
                    // 16 slots: centre cb of the block = register groups 2cb, 2cb+1 of both lane halves; slots
                    // 0-3 / 8-11 live in half 0, 4-7 / 12-15 in half 1.  This lane stores centre cb = h.
                    const float own0 = sums[0] + sums[1], own1 = sums[2] + sums[3];
                    const float mine = h ? own1 : own0;
                    const float theirs = h ? own0 : own1;
                    st_sum[rb][0] = mine + __shfl_xor(theirs, 32);
                    const int sh = 8 * h;
                    const unsigned int m16 = ((lo16 >> sh) & 0xFu) | (((hi16 >> sh) & 0xFu) << 4) |
                                             (((lo16 >> (sh + 4)) & 0xFu) << 8) | (((hi16 >> (sh + 4)) & 0xFu) << 12);
                    st_msk |= m16 << (16 * rb);
                }
            }
        }

        if (!wave_on && NI_B > 0) {                         // idle-column waves still stage their share
            GN_V2_WRITE_H(buf ^ 1, 0, CH_A, NI_A);
            GN_V2_GATHER_WIN(ic_n, jc_n, CH_A, CHUNKS, NI_B);
        }
        if (NI_B > 0) { GN_V2_WRITE_H(buf ^ 1, CH_A, CHUNKS, NI_B); }
        else { GN_V2_WRITE_H(buf ^ 1, 0, CH_A, NI_A); }
        if (gc0 == 0) s_jc[buf ^ 1][grow] = jc_n;
        ic_n = ic_nn; jc_n = ok_nn ? raw_nn : -1;
        // Output stores LAST: vmcnt retires in order, so any gathered operand consumed after a store would
        // also wait for that store's write acknowledgement.
        if (wave_on) {
            const long long c0t = (long long)tile * (V2_ROWS / S);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int c2 = 0; c2 < NST; ++c2) {
                    const long long centre = c0t + rb * (32 / S) + NST * h + c2;
                    if (centre < g.N) {
                        out[centre * ldo + col] = (__bf16)st_sum[rb][c2];
                        if constexpr (S == 8)
                            maskB[centre * H2 + col] = (unsigned char)(st_msk >> (8 * (2 * rb + c2)));
                        else
                            reinterpret_cast<unsigned short*>(maskB)[centre * H2 + col] = (unsigned short)(st_msk >> (16 * rb));
                        if (is_coord) coords[centre * 8 + coord_d] = st_sum[rb][c2];
                    }
                }
        }
        __syncthreads();
    }
#undef GN_V2_WRITE_H
}

// ---- forward epilogue of one 32-row block (one wave, 32 columns): relu, slot sums, slot masks.
// lane (r = column, h): registers 4c..4c+3 = rows 8c + 4h + (0..3).  vrow: bit (row - 4h) = row valid.
// S = 8: the block holds 4 centres x 8 slots; this lane returns centres 2h, 2h+1: ssum[0..1], smsk = 2 bytes.
// S = 16: 2 centres x 16 slots; this lane returns centre h: ssum[0], smsk = 16 bits.
__device__ __forceinline__ unsigned int xor32_u(unsigned int x, int h) {
    const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);    // {(lo, lo), (hi, hi)}: no LDS crossbar
    return h ? sw[0] : sw[1];
}
__device__ __forceinline__ float xor32_f(float x, int h) {
    return __builtin_bit_cast(float, xor32_u(__builtin_bit_cast(unsigned int, x), h));
}
// The epilogue is written as 8 element-pair steps + a combine so that a caller can place the pieces between MFMAs.
// Two fp32 partial sums per centre group (even / odd rows).  The bias add and the accumulation are plain fp32
// instructions on purpose (packed fp32 costs more issue time beside MFMAs than the two instructions it replaces).
struct FwdEpi { float sums[4][2]; unsigned int pack; };
__device__ __forceinline__ void fwd_epi_init(FwdEpi& e) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { e.sums[c][0] = 0.0f; e.sums[c][1] = 0.0f; }
    e.pack = 0;
}
// elements q, q-1 (q odd; call in the order q = 15, 13, .. 1).  The chain runs on the NEGATED weights, so
// y = -(pre-activation): relu(x) = -min(y, 0) and [x > 0] is the sign bit of y as it stands (y = -0.0 cannot
// occur: y = acc + nbias with nbias = -b2 added last, and a + b is -0.0 only for (-0.0) + (-0.0)).
// LEAKY (DynEdgeJINST): the second activation is a leaky relu: leaky(x) = max(x, 0.01 x) = -min(y, 0.01 y); the slot bit is
// still [x > 0] (torch's leaky_relu backward takes the slope at x <= 0); a row that does not exist enters as y = +0.0
// (adds nothing, bit clear) and is told apart from a real row with x <= 0 by the tile's validity word in the backward.
template <bool FAST, bool LEAKY = false>
__device__ __forceinline__ void fwd_epi_pair(FwdEpi& e, float a_hi, float a_lo, f32x2 nbias2, unsigned int vrow, int q) {
    float y0, y1;
    add2_f32(a_hi, nbias2[0], a_lo, nbias2[1], y0, y1);        // plain adds: see add2_f32
    if constexpr (!FAST) {
        y0 = ((vrow >> acc_row(q, 0)) & 1u) ? y0 : (LEAKY ? 0.0f : 1.0f);
        y1 = ((vrow >> acc_row(q - 1, 0)) & 1u) ? y1 : (LEAKY ? 0.0f : 1.0f);
    }
    const float m0 = fminf(y0, LEAKY ? 0.01f * y0 : 0.0f), m1 = fminf(y1, LEAKY ? 0.01f * y1 : 0.0f);
    e.sums[q >> 2][0] -= m0;
    e.sums[q >> 2][1] -= m1;
    e.pack = __builtin_amdgcn_alignbit(e.pack, __builtin_bit_cast(unsigned int, y0), 31);
    e.pack = __builtin_amdgcn_alignbit(e.pack, __builtin_bit_cast(unsigned int, y1), 31);
}
template <int S>
__device__ __forceinline__ void fwd_epi_combine(const FwdEpi& e, int h, float (&ssum)[2], unsigned int& smsk) {
    float sums[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) sums[c] = e.sums[c][0] + e.sums[c][1];
    const unsigned int other = xor32_u(e.pack, h);
    const unsigned int lo16 = h ? other : e.pack, hi16 = h ? e.pack : other;   // slots 0-3 / 4-7
    if constexpr (S == 8) {
        smsk = 0;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const float mine = h ? sums[2 + cc] : sums[cc];
            const float theirs = h ? sums[cc] : sums[2 + cc];
            ssum[cc] = mine + xor32_f(theirs, h);
            const int sh = 4 * (2 * h + cc);
            smsk |= (((lo16 >> sh) & 0xFu) | (((hi16 >> sh) & 0xFu) << 4)) << (8 * cc);
        }
    } else {
        const float own0 = sums[0] + sums[1], own1 = sums[2] + sums[3];
        const float mine = h ? own1 : own0;
        const float theirs = h ? own0 : own1;
        ssum[0] = mine + xor32_f(theirs, h);
        ssum[1] = 0.0f;
        const int sh = 8 * h;
        smsk = ((lo16 >> sh) & 0xFu) | (((hi16 >> sh) & 0xFu) << 4) |
               (((lo16 >> (sh + 4)) & 0xFu) << 8) | (((hi16 >> (sh + 4)) & 0xFu) << 12);
    }
}
template <int S, bool FAST, bool LEAKY = false>
__device__ __forceinline__ void fwd_epi_block(const f32x16& acc, float nbias, unsigned int vrow, int h, float (&ssum)[2], unsigned int& smsk) {
    FwdEpi e;
    fwd_epi_init(e);
    const f32x2 nb2 = {nbias, nbias};
#pragma unroll
    for (int q = 15; q >= 1; q -= 2) { const float ah = acc[q], al = acc[q - 1]; fwd_epi_pair<FAST, LEAKY>(e, ah, al, nb2, vrow, q); }
    fwd_epi_combine<S>(e, h, ssum, smsk);
}
// one MFMA chain (32 rows x 32 columns, K = 16 * KSTEPS, A fragments from LDS ahead of use) with the
// epilogue of `pend` placed between the MFMAs: source order pinned after every step.
template <int KSTEPS, int S, bool FAST, bool LEAKY = false>
__device__ __forceinline__ void fwd_phase(const unsigned char* a, const bf16x8 (&w2)[KSTEPS], float nbias, f32x16& acc_out,
                                          const f32x16& pend, unsigned int vrow, int h, float (&ssum)[2], unsigned int& smsk) {
    constexpr int STRIDE = KSTEPS >= 16 ? 2 : 1;       // one element pair every STRIDE steps (8 pairs in all)
    f32x16 acc;                                     // starts at 0 (inline constant): the bias is added in the epilogue, a
    zero_acc(acc);                                  // bias-filled start value would sit in 16 more registers all loop long
    FwdEpi e;
    fwd_epi_init(e);
    const f32x2 nb2 = {nbias, nbias};
    constexpr int PF = KSTEPS >= 21 ? 1 : 2;          // A fragments in flight ahead of the MFMA (register budget)
    bf16x8 f[KSTEPS];
#pragma unroll
    for (int s = 0; s < PF; ++s) f[s] = *reinterpret_cast<const bf16x8*>(a + s * 32);
    bool combined = false;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        if (s + PF < KSTEPS) f[s + PF] = *reinterpret_cast<const bf16x8*>(a + (s + PF) * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[s], w2[s], acc, 0, 0, 0);
        if (s % STRIDE == 0 && s / STRIDE < 8) {
            const int q = 15 - 2 * (s / STRIDE);
            const float ah = pend[q], al = pend[q - 1];
            fwd_epi_pair<FAST, LEAKY>(e, ah, al, nb2, vrow, q);
        }
        if (s / STRIDE >= 8 && !combined) { fwd_epi_combine<S>(e, h, ssum, smsk); combined = true; }
        // pin the step: the accumulator chain and the epilogue state pass through an empty asm, so neither the
        // IR passes nor the instruction schedulers can sink the vector work behind the MFMA chain
        asm volatile("" : "+v"(acc), "+v"(e.pack), "+v"(e.sums[0]), "+v"(e.sums[1]), "+v"(e.sums[2]), "+v"(e.sums[3]));
        __builtin_amdgcn_sched_barrier(0);
    }
    if (!combined) fwd_epi_combine<S>(e, h, ssum, smsk);
    acc_out = acc;
}

// =============================================================================== forward, wave-specialised
// Same tile and operand layout as edge_fwd_v2_kernel (results equal up to the summation order of the slot sums).
// In the kernel above the two waves of a SIMD run gather / MFMA / epilogue phases in lockstep and the vector and
// matrix pipes take turns (co-execution 8 % of the cycles).  Here
//   * waves 8-11 = producers (one per SIMD): gather P[i], Q[j] of the tile after next (4 threads per edge row, the
//     loads are in flight for a whole tile), h = relu(P + Q) -> the other LDS buffer;
//   * waves 0-7  = consumers: stationary (negated) W2 slice, two 21-step MFMA chains per tile (rows 0-31, 32-63)
//     read from the LDS tile, and BETWEEN the MFMAs of a chain the relu / slot-sum / slot-mask epilogue of the
//     previous chain's accumulators (fwd_phase): vector instructions of the same wave issue in the free slots of
//     its MFMAs, vector work of another wave does not (measured: DESIGN.md section 5).
// One barrier per tile; 12 waves = 3 per SIMD (VGPR budget 168: W2 slice 84, two accumulator tiles 32).
constexpr int WS_THREADS = 768;
// KSTEPS = H1p / 16 (row layout of P|Q and W2p), KUSE = ceil(H1 / 16) <= KSTEPS: the k-steps that hold real columns
// (H1 = 336: 21 of 22: the last one is the packed layout's zero padding and is neither gathered nor multiplied).
// ---- EdgeConvTito epilogue of one 32-row block: max over a centre's valid slots of (acc + b2), the slot that
// supplied it (first maximum in slot order, as csrc/generic.hip: slot_reduce_kernel), then leaky relu of the maximum (a
// strictly increasing activation commutes with max).  Returns this lane's centres (S = 8: 2h, 2h+1; S = 16: h):
// value (0 when the centre has no edge in these slots) and the ONE-HOT slot mask (0 = none) - the backward kernels
// read it exactly like the relu slot masks: d(out)/d(row) is non-zero on the arg row only.
template <int S>
__device__ __forceinline__ void max_epi_block(const f32x16& acc, float bias, unsigned int vrow, int h, float (&sval)[2],
                                              unsigned int& smsk) {
    float gm[4];
    int ga[4];                                         // per register group c: max / slot (within the group) / -1
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float m = -3.0e38f;
        int a = -1;
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int q = 4 * c + qq;
            const bool ok = (vrow >> acc_row(q, 0)) & 1u;
            const float v = acc[q] + bias;
            if (ok && v > m) { m = v; a = qq; }
        }
        gm[c] = m; ga[c] = a;
    }
    smsk = 0;
    if constexpr (S == 8) {
        // group c = centre c of the block: this half holds slots 4h .. 4h+3, the partner half the other four
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            // this lane stores centre 2h + cc and needs the partner half's four slots of it; it sends its own slots of
            // the centre the partner stores, 2(1-h) + cc (selects, not a per-lane register index)
            const float mine_m = h ? gm[2 + cc] : gm[cc], send_m = h ? gm[cc] : gm[2 + cc];
            const int mine_a = h ? ga[2 + cc] : ga[cc], send_a = h ? ga[cc] : ga[2 + cc];
            const float pm = xor32_f(send_m, h);
            const int pa = (int)xor32_u((unsigned int)send_a, h);
            const float lo_m = h ? pm : mine_m, hi_m = h ? mine_m : pm;     // slots 0-3 / 4-7 in slot order
            const int lo_a = h ? pa : mine_a, hi_a = h ? mine_a : pa;
            float m = lo_m;
            int a = lo_a;
            if (hi_a >= 0 && (a < 0 || hi_m > m)) { m = hi_m; a = hi_a + 4; }
            sval[cc] = a >= 0 ? fmaxf(m, 0.01f * m) : 0.0f;
            smsk |= (a >= 0 ? (1u << a) : 0u) << (8 * cc);
        }
    } else {
        // 16 slots: centre cb = groups 2cb, 2cb+1 of both halves; slot order: h0.g(2cb) 0-3, h1.g(2cb) 4-7, h0.g(2cb+1)
        // 8-11, h1.g(2cb+1) 12-15.  This lane stores centre cb = h.
        const float m0 = h ? gm[2] : gm[0], m1 = h ? gm[3] : gm[1];          // my slots of MY centre (cb = h): groups 2h, 2h+1
        const int a0 = h ? ga[2] : ga[0], a1 = h ? ga[3] : ga[1];
        const float s0 = h ? gm[0] : gm[2], s1 = h ? gm[1] : gm[3];          // my slots of the PARTNER's centre (1 - h)
        const int t0 = h ? ga[0] : ga[2], t1 = h ? ga[1] : ga[3];
        const float p0m = xor32_f(s0, h), p1m = xor32_f(s1, h);
        const int p0a = (int)xor32_u((unsigned int)t0, h), p1a = (int)xor32_u((unsigned int)t1, h);
        const float o_m[4] = {h ? p0m : m0, h ? m0 : p0m, h ? p1m : m1, h ? m1 : p1m};
        const int o_a[4] = {h ? p0a : a0, h ? a0 : p0a, h ? p1a : a1, h ? a1 : p1a};
        float m = -3.0e38f;
        int a = -1;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (o_a[t] >= 0 && (a < 0 || o_m[t] > m)) { m = o_m[t]; a = o_a[t] + 4 * t; }
        sval[0] = a >= 0 ? fmaxf(m, 0.01f * m) : 0.0f;
        sval[1] = 0.0f;
        smsk = a >= 0 ? (1u << a) : 0u;
    }
}

template <int KSTEPS, int KUSE, int S, int V = 0>
__global__ __launch_bounds__(WS_THREADS) void edge_fwd_ws_kernel(
    EdgeGraph g, const __bf16* __restrict__ PQ, const __bf16* __restrict__ W2p, const float* __restrict__ b2,
    int H2, __bf16* __restrict__ out, long long ldo, float* __restrict__ coords, CoordCols ccols,
    unsigned char* __restrict__ maskB, int ntiles, int producers_first, unsigned long long* __restrict__ tilevalid)
{
    static_assert(S == 8 || S == 16, "8 or 16 slots per centre");
    constexpr int NST = 16 / S;
    constexpr int K = KSTEPS * 16;
    constexpr int ROWB = K * 2 + 16;
    constexpr bool LEAKY = V == 2;
    constexpr int CHUNKS = KUSE * 2;                   // 16-byte chunks per row that are gathered
    __shared__ __attribute__((aligned(16))) unsigned char As[2][V2_ROWS * ROWB];
    __shared__ int s_jc[2][V2_ROWS];

    // producers_first (A/B switch GN_WS_PRODUCERS_FIRST): the producer role goes to waves 0-3 (the OLDEST waves of the
    // workgroup win the vector-issue arbitration of their SIMD) instead of 8-11; `wave` below is the role index:
    // 0-7 consumers, 8-11 producers, whichever hardware waves play them
    const int tid = threadIdx.x, lane = tid & 63, hw_wave = tid >> 6;
    const int wave = producers_first ? (hw_wave < 4 ? hw_wave + 8 : hw_wave - 4) : hw_wave;
    const long long main_rows = (long long)g.N * S;
    const int kslots = g.K;
    const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    int tile = blockIdx.x * per;
    const int tile_end = min(ntiles, tile + per);

    if (wave >= 8) {
        // ------------------------------------------------------------------ producer
        constexpr int NI = (CHUNKS + 3) / 4;             // 16-byte chunks per thread (4 threads per row)
        const int ptid = (wave - 8) * 64 + lane;
        const int grow = ptid >> 2, gc0 = ptid & 3;
        u32x4 preg[NI], qreg[NI];
        // 32-bit byte offsets off the uniform base; chunk i sits at the immediate offset 64 * i from the thread's first
        // chunk, except that the last round is clamped into the row (4 * NI may exceed CHUNKS)
        const unsigned char* PQb = reinterpret_cast<const unsigned char*>(PQ);
        constexpr unsigned int ROWPQ = 2u * K * 2u;
        const unsigned int clast = (gc0 + 4 * (NI - 1) < CHUNKS ? gc0 + 4 * (NI - 1) : CHUNKS - 1) * 16u;
#define GN_WS_GATHER(ic_, jc_)                                                                        \
    {                                                                                                 \
        const unsigned int js__ = (jc_) < 0 ? 0u : (unsigned int)(jc_);                               \
        const unsigned int po__ = __umul24((unsigned int)(ic_), ROWPQ);                               \
        const unsigned int qo__ = __umul24(js__, ROWPQ) + 2u * K;                                     \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                              \
            const unsigned int co__ = (i + 1 < NI) ? (unsigned int)gc0 * 16u + 64u * i : clast;       \
            preg[i] = *reinterpret_cast<const u32x4*>(PQb + po__ + co__);                             \
            qreg[i] = *reinterpret_cast<const u32x4*>(PQb + qo__ + co__);                             \
        }                                                                                             \
    }
#define GN_WS_WRITE_H(buf_)                                                                           \
    {                                                                                                 \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                              \
            const unsigned int co__ = (i + 1 < NI) ? (unsigned int)gc0 * 16u + 64u * i : clast;       \
            *reinterpret_cast<u32x4*>(&As[buf_][grow * ROWB + co__]) = act_sum_bf16x8<V>(preg[i], qreg[i]); \
        }                                                                                             \
    }
        int ic_n, jc_n;                                   // row info of the tile whose chunks are in flight
        {
            int ic, jc;
            GN_V2_INFO(tile, ic, jc);
            GN_WS_GATHER(ic, jc);
            GN_V2_INFO(tile + 1, ic_n, jc_n);
            GN_WS_WRITE_H(0);
            if (gc0 == 0) s_jc[0][grow] = jc;
            GN_WS_GATHER(ic_n, jc_n);
        }
        __syncthreads();
        int buf = 0;
        for (; tile < tile_end; ++tile, buf ^= 1) {
            int ic_nn, raw_nn;
            bool ok_nn;
            GN_V2_INFO_ISSUE(tile + 2, ic_nn, raw_nn, ok_nn);     // issued before, consumed after the tile's work
            GN_WS_WRITE_H(buf ^ 1);                               // chunks of tile + 1 (loaded one tile ago)
            if (gc0 == 0) s_jc[buf ^ 1][grow] = jc_n;
            ic_n = ic_nn; jc_n = ok_nn ? raw_nn : -1;
            GN_WS_GATHER(ic_n, jc_n);                             // tile + 2: lands while the consumers run tile + 1
            __syncthreads();
        }
#undef GN_WS_GATHER
#undef GN_WS_WRITE_H
        return;
    }

    // ---------------------------------------------------------------------- consumer
    // Software pipeline: the epilogue (vector ALU) of one 32-row block is interleaved, instruction by
    // instruction, with the MFMA chain of the NEXT block of the same wave (phase A: rows 0-31 of tile t beside
    // the epilogue of rows 32-63 of tile t-1; phase B: rows 32-63 beside the epilogue of rows 0-31), so the
    // vector instructions issue in the 24 free cycles of every 32-cycle MFMA slot instead of after the chain.
    const int r = lane & 31, h = lane >> 5;
    const bool wave_on = wave * 32 < H2;
    bf16x8 w2[KUSE];                                 // NEGATED W2 slice (see fwd_epi_elem)
#pragma unroll
    for (int s = 0; s < KUSE; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) w2[s][e] = (__bf16)0.0f;
    if (wave_on) {
        const __bf16* wrow = W2p + (long long)(wave * 32 + r) * K + h * 8;
#pragma unroll
        for (int s = 0; s < KUSE; ++s) {
            constexpr unsigned int NEG = V != 1 ? 0x80008000u : 0u;      // the relu / leaky-sum epilogue runs on negated weights
            const u32x4 wv = *reinterpret_cast<const u32x4*>(wrow + s * 16) ^ (u32x4){NEG, NEG, NEG, NEG};
            w2[s] = __builtin_bit_cast(bf16x8, wv);
        }
    }
    const int col = wave * 32 + r;
    const float bias = (col < H2) ? (V != 1 ? -b2[col] : b2[col]) : 0.0f;     // negated with the weights
    int coord_d = -1;
#pragma unroll
    for (int d = 0; d < 8; ++d)
        if (coords && d < ccols.n && ccols.c[d] == col) coord_d = d;
    const bool is_coord = coord_d >= 0;
    const int tile0 = tile;
    __syncthreads();

    // stores of one row block's results: S = 8: centres 2h, 2h+1 of the block; S = 16: centre h
#define GN_WS_STORE(tile_, rb_, ssum_, smsk_)                                                         \
    {                                                                                                 \
        const int c0t__ = (tile_) * (V2_ROWS / S) + (rb_) * (32 / S) + NST * h;                       \
        _Pragma("unroll") for (int c2 = 0; c2 < NST; ++c2) {                                          \
            const int centre = c0t__ + c2;                 /* 32-bit element offsets off uniform bases */ \
            if (centre < g.N) {                                                                       \
                out[(unsigned int)centre * ldo32 + (unsigned int)col] = (__bf16)ssum_[c2];            \
                const unsigned int mo__ = (unsigned int)centre * (unsigned int)H2 + (unsigned int)col; \
                if constexpr (S == 8) maskB[mo__] = (unsigned char)((smsk_) >> (8 * c2));              \
                else reinterpret_cast<unsigned short*>(maskB)[mo__] = (unsigned short)(smsk_);        \
                if (is_coord) coords[(unsigned int)centre * 8u + (unsigned int)coord_d] = ssum_[c2];  \
            }                                                                                         \
        }                                                                                             \
    }
    const unsigned int ldo32 = (unsigned int)ldo;

    if constexpr (V == 1) {
        // EdgeConvTito: plain chain, then the max / arg epilogue (no pending block, no validity fast path)
        int bufm = 0;
        for (; tile < tile_end; ++tile, bufm ^= 1) {
            if (wave_on) {
                const unsigned long long vbits = __ballot(s_jc[bufm][lane] >= 0);
                const unsigned char* a0 = &As[bufm][r * ROWB + h * 16];
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f32x16 acc;
                    zero_acc(acc);
#pragma unroll
                    for (int s = 0; s < KUSE; ++s)
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(a0 + rb * 32 * ROWB + s * 32),
                                                                      w2[s], acc, 0, 0, 0);
                    float sval[2];
                    unsigned int smsk;
                    max_epi_block<S>(acc, bias, (unsigned int)(vbits >> (32 * rb + 4 * h)), h, sval, smsk);
                    GN_WS_STORE(tile, rb, sval, smsk);
                }
            }
            __syncthreads();
        }
        return;
    }
    f32x16 accP;                                     // rows 32-63 of the previous tile, epilogue pending
    zero_acc(accP);
    unsigned int vrowP = 0;
    bool fastP = true;                               // wave-uniform: every row of the pending block is valid
    int buf = 0;
    for (; tile < tile_end; ++tile, buf ^= 1) {
        if (wave_on) {
            const unsigned long long vbits = __ballot(s_jc[buf][lane] >= 0);      // bit = tile row valid
            if (LEAKY && wave == 0 && lane == 0) tilevalid[tile] = vbits;         // the backward kernels' row validity
            const unsigned char* a0 = &As[buf][r * ROWB + h * 16];
            f32x16 acc1;
            // Rows are invalid only in events of fewer than 9 pulses and in the last tile: two code paths, the hot
            // one without any per-element validity select, the rare one plain (chain, then epilogue).
            if (fastP && (unsigned int)vbits == 0xffffffffu) {
                f32x16 acc0;
                float sumP[2], sum0[2];
                unsigned int mskP, msk0;
                fwd_phase<KUSE, S, true, LEAKY>(a0, w2, bias, acc0, accP, 0u, h, sumP, mskP);
                // consumer waves issue no global loads: their stores go out at once (nothing of theirs waits on vmcnt)
                if (tile > tile0) GN_WS_STORE(tile - 1, 1, sumP, mskP);
                fwd_phase<KUSE, S, true, LEAKY>(a0 + 32 * ROWB, w2, bias, acc1, acc0, 0u, h, sum0, msk0);
                GN_WS_STORE(tile, 0, sum0, msk0);
            } else {
                float ssum[2];
                unsigned int smsk;
                if (tile > tile0) {
                    fwd_epi_block<S, false, LEAKY>(accP, bias, vrowP, h, ssum, smsk);
                    GN_WS_STORE(tile - 1, 1, ssum, smsk);
                }
                f32x16 acc0;
                zero_acc(acc0);
#pragma unroll
                for (int s = 0; s < KUSE; ++s)
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(a0 + s * 32), w2[s], acc0, 0, 0, 0);
                fwd_epi_block<S, false, LEAKY>(acc0, bias, (unsigned int)(vbits >> (4 * h)), h, ssum, smsk);
                GN_WS_STORE(tile, 0, ssum, smsk);
                zero_acc(acc1);
#pragma unroll
                for (int s = 0; s < KUSE; ++s)
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(a0 + 32 * ROWB + s * 32), w2[s], acc1, 0, 0, 0);
            }
            accP = acc1;
            vrowP = (unsigned int)(vbits >> (32 + 4 * h));
            fastP = (unsigned int)(vbits >> 32) == 0xffffffffu;
        }
        __syncthreads();
    }
    if (wave_on && tile_end > tile0) {               // drain: rows 32-63 of the last tile
        float sumP[2];
        unsigned int mskP;
        fwd_epi_block<S, false, LEAKY>(accP, bias, vrowP, h, sumP, mskP);
        GN_WS_STORE(tile_end - 1, 1, sumP, mskP);
    }
#undef GN_WS_STORE
}

// =============================================================================== dW2 / db2 / hbits
// LDS pitch for tiles read with ds_read_b64_tr_b16: 4 consecutive rows must hit disjoint 64-byte
// bank ranges -> pitch == 64 (mod 256).
__host__ __device__ constexpr int tr_pitch(int row_bytes) {
    return row_bytes + ((64 - row_bytes % 256) + 256) % 256;
}

// pitch >= row_bytes, multiple of 8 bytes, (pitch / 4) mod 32 == 18: see edge_bwd_v2_kernel
__host__ __device__ constexpr int stage_pitch(int row_bytes) {
    int p = (row_bytes + 7) / 8 * 8;
    while ((p / 4) % 32 != 18) p += 8;
    return p;
}

// =============================================================================== dW2 / db2 / hbits, software-pipelined
// dW2[H2][H1] = dm^T h over the table's edge rows, written as partial slabs (one per tile range) with db2 = column sums of
// dm, and the h > 0 bits the backward kernel reads.  The k1 (= H1p) range is split over HALVES workgroup populations so
// that the stationary accumulator (32 x NBH*32 fp32 per wave) fits the 256-VGPR budget of 2 waves/SIMD: workgroup b
// handles k1 blocks [kb0, kb0+nblk) (kb0 = (b % HALVES) * NBH) of the tile range b / HALVES, gathers only those columns
// of h, and writes them into slab b / HALVES.
// The kernel this one replaced was barrier-phased: the two waves of a SIMD met at the tile barrier and then ran the same
// program, first their MFMAs (with a wait on LDS at every k-step), then ~150 vector instructions with the matrix pipe idle
// (s_memtime probe: 3.4k cycles per tile against 1.5k of MFMA and 1.5k of vector issue per SIMD - they do not overlap
// ACROSS waves: an MFMA that waits for the pipe holds the SIMD's vector issue, so only a wave's OWN vector instructions
// ride in the shadow of its MFMAs).  Here every iteration is ONE straight-line block:
//   * iteration T multiplies tile T (h in LDS, dm^T fragments ready in registers) and meanwhile
//       - builds h of tile T+1 from chunks gathered during iteration T-1 and re-issues each chunk's loads for tile T+2
//         as soon as its registers are free (a full iteration of latency cover with one register set),
//       - builds the dm^T fragments of tile T+1 from g_out / slot bytes loaded during iteration T-1, loads those of T+2,
//       - reads the h^T fragment of a later MFMA while the current one runs (rolling window, counted waits);
//   * NW = 4 waves (ONE per SIMD, 512 registers): a wave owns NA = 2 column blocks of dm, so an h^T fragment read from
//     LDS feeds two MFMAs and the wave has 2 x NBLK independent accumulators; NW = 8 (what runs): two waves per SIMD, one column block each;
//   * no branch in the loop: look-ahead tiles past the end are clamped (loads) or land in slack rows (hbits stores,
//     saved_layout() keeps two tiles of slack), invalid centres of the last tile are cut by one byte mask per tile;
//   * the k1 block count of the workgroup is a template parameter (the half is chosen once, at kernel entry);
//   * db2 = column sums of dm: when the h tile has a whole 8-column pad chunk (ceil(H1/8)*8 < H1p) its first column is
//     set to 1.0 once and the MFMAs deliver db2 as that column of dW2 (BSUM = false); otherwise 3 instructions per
//     k-step on the vector ALU (BSUM = true).
// What did NOT help (B = 4096, ms per launch, this kernel 1.25): sched_group_barrier patterns "1 MFMA, 2 LDS reads, n
// vector instructions" (1.5-2.3: the pass also displaces the look-ahead loads), fenced matrix / vector sections with the
// SIMD partners in opposite phases (1.34), one scheduling region per k-step (1.25), s_setprio 1 for waves 4-7 (1.25),
// NW = 4 (1.58: one wave's stream alone does not keep both pipes busy as the compiler orders it).
template <int NB1, int NBH, int S, int V, int NBLK, bool BSUM, int NW>
__device__ __forceinline__ void edge_dw2_v3_body(
    const EdgeGraph& g, const unsigned char* __restrict__ PQb, const int H1, const int H2,
    const unsigned char* __restrict__ goutb, const unsigned int ldg2, const unsigned char* __restrict__ maskB,
    unsigned char* __restrict__ hbits, float* __restrict__ slab, float* __restrict__ db2_part, const int ntiles,
    const int part, const int nparts, const int kb0, unsigned char* __restrict__ Hs, const unsigned char* __restrict__ MaskLut,
    const unsigned long long* __restrict__ tilevalid)
{
    static_assert(NW == 4 || NW == 8, "one or two waves per SIMD");
    constexpr int NT = NW * 64;                     // threads
    constexpr int TPR = NT / V2_ROWS;               // threads per h row
    constexpr int NA = 8 / NW;                      // dm column blocks per wave
    constexpr int K = NB1 * 32;
    constexpr int CHUNKS = K / 8;
    constexpr int NI = (NBLK * 4 + TPR - 1) / TPR;  // 16-byte chunks per thread
    constexpr int HP = tr_pitch(NBH * 64);
    constexpr int BUFSZ = V2_ROWS * HP;
    constexpr int CPT = V2_ROWS / S;                // centres per tile
    constexpr unsigned int ROWPQ = 2u * K * 2u;     // bytes per P|Q row
    constexpr int NQ = 4 * NBLK;                    // h^T fragments per tile and wave (each feeds NA MFMAs)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int kslots = g.K;
    const int n2 = wave * (32 * NA) + r;            // first dm column of this lane (A rows): n2 + 32 a, a < NA; H2 == 256
    const int cbeg = kb0 * 4;
    const int cend_all = (kb0 + NBLK) * 4;
    const int creal = (H1 + 7) / 8;
    const int cend = cend_all < creal ? cend_all : creal;

    f32x16 acc[NA][NBLK];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb) zero_acc(acc[a][nb]);
    float bsum[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) bsum[a] = 0.0f;

    // ---- per-thread constants of the h build (TPR threads per row)
    const int grow = tid / TPR, gc0 = tid % TPR;
    const int sl = grow % S, slc = sl < kslots ? sl : 0;
    unsigned int c16[NI], ldsw[NI], cix[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = cbeg + gc0 + TPR * i;
        const int cc = c < cend ? c : cend - 1;
        cix[i] = (unsigned int)cc;
        c16[i] = (unsigned int)cc * 16u;
        ldsw[i] = (unsigned int)(grow * HP + (cc - cbeg) * 16);
    }
    // pad columns of the window: zero once in both buffers; the first column of chunk `creal` (if in this window) is 1.0
    for (int idx = tid; idx < 2 * V2_ROWS * (cend_all - cend); idx += NT) {
        const int bufz = idx / (V2_ROWS * (cend_all - cend)), rem = idx % (V2_ROWS * (cend_all - cend));
        const int rowz = rem / (cend_all - cend), cz = cend + rem % (cend_all - cend);
        u32x4 z = {0u, 0u, 0u, 0u};
        if (!BSUM && cz == creal) z[0] = 0x00003f80u;
        *reinterpret_cast<u32x4*>(&Hs[bufz * BUFSZ + rowz * HP + (cz - cbeg) * 16]) = z;
    }

    const int per = (ntiles + nparts - 1) / nparts;
    int tile = part * per;
    const int tile_end = min(ntiles, tile + per);
    const unsigned int Nm1 = (unsigned int)(g.N - 1);

    // centre of this thread's build row in tile t, clamped to a real node (look-ahead tiles, last tile)
    auto build_centre = [&](int t) -> unsigned int {
        const unsigned int c = (unsigned int)(t * CPT + grow / S);
        return c < Nm1 ? c : Nm1;
    };
    auto nbr_of = [&](unsigned int c) -> int { return g.nbr[__umul24(c, (unsigned int)kslots) + (unsigned int)slc]; };
    u32x4 preg[NI], qreg[NI];
    auto gather_chunk = [&](int i, unsigned int po, unsigned int qo) {
        preg[i] = *reinterpret_cast<const u32x4*>(PQb + (po + c16[i]));
        qreg[i] = *reinterpret_cast<const u32x4*>(PQb + (qo + c16[i]));
    };
    auto row_offsets = [&](unsigned int c, int raw, unsigned int& po, unsigned int& qo) {
        const unsigned int js = (unsigned int)(raw < 0 ? 0 : raw);
        po = __umul24(c, ROWPQ);
        qo = __umul24(js, ROWPQ) + 2u * K;
    };
    // A side of tile t: g_out bits (bf16 in the low half) and the four slot bytes of this lane and column, packed.  The
    // tile part of every address is uniform (scalar unit); per lane: one add + one clamp for g_out (a look-ahead tile or
    // the last tile may name centres >= N; their slot bytes are cut by valid_bytes(), the mask rows read there are slack
    // of `saved`)
    const unsigned int gmax = Nm1 * ldg2 + (unsigned int)n2 * 2u;
    const unsigned int lane_goff = (S == 8 ? (unsigned int)h * ldg2 : 0u) + (unsigned int)n2 * 2u;
    const unsigned int lane_moff = S == 8 ? (unsigned int)(h * H2 + n2) : (unsigned int)(n2 * 2 + h);
    // V = 2: vm = the validity bytes of this lane's four k-steps (k-step s, lane half h: rows 16 s + 8 h .. + 7 of the tile)
    auto load_a = [&](int t, unsigned int (&gv)[NA][4], unsigned int (&mv)[NA], unsigned int& vm) {
        const int tc = t < ntiles ? t : ntiles - 1;                      // uniform
        if constexpr (V == 2) {
            const unsigned long long vw = tilevalid[tc];                 // uniform: scalar load
            const unsigned int xl = (unsigned int)vw >> (8 * h), xh = (unsigned int)(vw >> 32) >> (8 * h);
            vm = (xl & 0xffu) | ((xl >> 8) & 0xff00u) | ((xh & 0xffu) << 16) | ((xh << 8) & 0xff000000u);
        } else {
            vm = 0u;
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) mv[a] = 0u;
#pragma unroll
        for (int s = 3; s >= 0; --s) {
            const unsigned int cs = (unsigned int)(tc * CPT + (S == 8 ? 2 * s : s));     // uniform
            unsigned int go = cs * ldg2 + lane_goff;
            go = go < gmax ? go : gmax;
            const unsigned int mo = cs * (unsigned int)(S == 8 ? H2 : 2 * H2) + lane_moff;    // uniform product + lane
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                gv[a][s] = (unsigned int)*reinterpret_cast<const unsigned short*>(goutb + go + 64u * a);
                mv[a] = (mv[a] << 8) | (unsigned int)maskB[mo + (S == 8 ? 32u : 64u) * a];
            }
        }
    };
    // byte mask of the k-steps whose centre exists (tile t; all ones except in the last tile and beyond)
    auto valid_bytes = [&](int t, bool mine) -> unsigned int {
        const int nv = mine ? g.N - t * CPT : 0;                         // uniform
        int ns0, ns1;
        if (S == 8) { ns0 = (nv + 1) >> 1; ns1 = nv >> 1; } else { ns0 = nv; ns1 = nv; }
        ns0 = ns0 < 0 ? 0 : (ns0 > 4 ? 4 : ns0);
        ns1 = ns1 < 0 ? 0 : (ns1 > 4 ? 4 : ns1);
        const unsigned int b0 = ns0 >= 4 ? 0xffffffffu : ((1u << (8 * ns0)) - 1u);
        const unsigned int b1 = ns1 >= 4 ? 0xffffffffu : ((1u << (8 * ns1)) - 1u);
        return h ? b1 : b0;
    };
    // dm fragment of one k-step: g_out where the slot bit is set; V = 2 (leaky second activation): 0.01 g_out on the
    // slots in `inv` (row exists, bit clear); bs: this k-step's share of db2 (BSUM)
    auto make_afrag = [&](unsigned int gbits, unsigned int m, unsigned int inv, float& bs) -> bf16x8 {
        const unsigned int gbf = gbits | (gbits << 16);
        const u32x4 mk = *reinterpret_cast<const u32x4*>(&MaskLut[m * 16]);
        const u32x4 gb4 = {gbf, gbf, gbf, gbf};
        u32x4 aw = gb4 & mk;
        const float gf = __builtin_bit_cast(float, gbits << 16);
        if (BSUM) bs += gf * (float)__builtin_popcount(m);
        if constexpr (V == 2) {
            const float gs = 0.01f * gf;
            const unsigned int sb = pack_bf16x2(gs, gs);
            // (a branch "every slot exists: sb4 & ~mk, no second look-up" inside this software-pipelined loop cost 15 %)
            const u32x4 mi = *reinterpret_cast<const u32x4*>(&MaskLut[inv * 16]);
            aw |= (u32x4){sb, sb, sb, sb} & mi;
            if (BSUM) bs += __builtin_bit_cast(float, sb << 16) * (float)__builtin_popcount(inv);
        }
        return __builtin_bit_cast(bf16x8, aw);
    };

    if (tile < tile_end) {
        // ---------------- prologue: h(tile) in buffer 0, chunks of tile+1 in flight, fragments of tile ready
        bf16x8 afrag[NA][4];
        unsigned int gb1[NA][4], mw1[NA], vm1;
        unsigned int c2;            // centre / neighbour of this thread's build row in tile+2
        int raw2;
        {
            const unsigned int c0 = build_centre(tile), c1 = build_centre(tile + 1);
            const int raw0 = nbr_of(c0), raw1 = nbr_of(c1);
            c2 = build_centre(tile + 2);
            raw2 = nbr_of(c2);
            unsigned int ga0[NA][4], mw0[NA], vm0;
            load_a(tile, ga0, mw0, vm0);
            load_a(tile + 1, gb1, mw1, vm1);
            unsigned int po, qo;
            row_offsets(c0, raw0, po, qo);
#pragma unroll
            for (int i = 0; i < NI; ++i) gather_chunk(i, po, qo);
            const unsigned int hrow = (unsigned int)(tile * V2_ROWS + grow) * (unsigned int)CHUNKS;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const u32x4 hv = act_sum_bf16x8<V>(preg[i], qreg[i]);
                *reinterpret_cast<u32x4*>(&Hs[ldsw[i]]) = hv;
                hbits[hrow + cix[i]] = (unsigned char)(V == 0 ? nonzero_bits_bf16x8(hv) : positive_bits_bf16x8(hv));
            }
            row_offsets(c1, raw1, po, qo);
#pragma unroll
            for (int i = 0; i < NI; ++i) gather_chunk(i, po, qo);
            const unsigned int vb = valid_bytes(tile, true);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                mw0[a] &= vb;
                const unsigned int iv = vm0 & vb & ~mw0[a];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const unsigned int m = (mw0[a] >> (8 * s)) & 0xffu;
                    afrag[a][s] = make_afrag(ga0[a][s], m, (iv >> (8 * s)) & 0xffu, bsum[a]);
                }
            }
        }
        __syncthreads();

        const int g4 = lane >> 4, li = lane & 15;
        const unsigned int tr_base = (unsigned int)((8 * (g4 >> 1) + (li >> 2)) * HP + (16 * (g4 & 1) + 4 * (li & 3)) * 2);
        unsigned int hrow1 = (unsigned int)((tile + 1) * V2_ROWS + grow) * (unsigned int)CHUNKS;   // hbits row offset of tile+1

        int buf = 0;
        for (; tile < tile_end; ++tile, buf ^= 1) {
            typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
            // look-ahead loads: neighbour of tile+3, A side of tile+2
            const unsigned int c3 = build_centre(tile + 3);
            const int raw3 = nbr_of(c3);
            unsigned int gb2[NA][4], mw2[NA], vm2;
            load_a(tile + 2, gb2, mw2, vm2);
            unsigned int po2, qo2;
            row_offsets(c2, raw2, po2, qo2);
            const unsigned char* hb = Hs + (buf ? BUFSZ : 0) + tr_base;
            unsigned char* hw = Hs + (buf ? 0 : BUFSZ);
            const unsigned int vb1 = valid_bytes(tile + 1, tile + 1 < tile_end);   // (tile_end is not this workgroup's: no db2 from it)
#pragma unroll
            for (int a = 0; a < NA; ++a) mw1[a] &= vb1;

            constexpr int AHEAD = NW == 4 ? 3 : NBLK;       // fragments read ahead of the MFMAs that use them
            bf16x8 bfr[NQ];
            auto read_b = [&](int q) {
                const int s = q / NBLK, nb = q % NBLK;
                const unsigned char* p0 = hb + (16 * s) * HP + nb * 64;
                const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0));
                const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + 4 * HP));
                bfr[q] = __builtin_bit_cast(bf16x8, __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7));
            };
#pragma unroll
            for (int q = 0; q < AHEAD; ++q) read_b(q);

            bf16x8 anext[NA][4];
            unsigned int hbv[NI];
            constexpr int CSTEP = NQ / NI;                  // a chunk of h every CSTEP fragments
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int s = q / NBLK, nb = q % NBLK;
#pragma unroll
                for (int a = 0; a < NA; ++a)
                    acc[a][nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag[a][s], bfr[q], acc[a][nb], 0, 0, 0);
                if (q + AHEAD < NQ) read_b(q + AHEAD);
                // vector work in the shadow of the MFMAs: the h chunks spread over the tile, fragment s at the end of k-step s
                if (q % CSTEP == 0 && q / CSTEP < NI) {
                    const int i = q / CSTEP;
                    const u32x4 hv = act_sum_bf16x8<V>(preg[i], qreg[i]);
                    *reinterpret_cast<u32x4*>(&hw[ldsw[i]]) = hv;
                    hbv[i] = V == 0 ? nonzero_bits_bf16x8(hv) : positive_bits_bf16x8(hv);
                    gather_chunk(i, po2, qo2);
                }
                if (nb == NBLK - 1) {
#pragma unroll
                    for (int a = 0; a < NA; ++a) {
                        const unsigned int m = (mw1[a] >> (8 * s)) & 0xffu;
                        const unsigned int iv = ((vm1 & vb1 & ~mw1[a]) >> (8 * s)) & 0xffu;
                        anext[a][s] = make_afrag(gb1[a][s], m, iv, bsum[a]);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) hbits[hrow1 + cix[i]] = (unsigned char)hbv[i];
            hrow1 += (unsigned int)(V2_ROWS * CHUNKS);
#pragma unroll
            for (int a = 0; a < NA; ++a) {
#pragma unroll
                for (int s = 0; s < 4; ++s) { afrag[a][s] = anext[a][s]; gb1[a][s] = gb2[a][s]; }
                mw1[a] = mw2[a];
            }
            vm1 = vm2;
            c2 = c3; raw2 = raw3;
            __syncthreads();
        }
    }

    // ---- write this workgroup's part of slab `part`: dW2[H2][k1 window]; db2[H2] from the ones column or the sums
    {
        float* outp = slab + (long long)part * H2 * H1;
#pragma unroll
        for (int nb = 0; nb < NBLK; ++nb) {
            const int k1 = (kb0 + nb) * 32 + r;
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                if (k1 < H1) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = wave * (32 * NA) + 32 * a + acc_row(q, h);
                        outp[(long long)row * H1 + k1] = acc[a][nb][q];
                    }
                } else if (!BSUM && k1 == creal * 8) {
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        db2_part[(long long)part * H2 + wave * (32 * NA) + 32 * a + acc_row(q, h)] = acc[a][nb][q];
                }
            }
        }
        if (BSUM) {
#pragma unroll
            for (int a = 0; a < NA; ++a) {
                const float bs = bsum[a] + __shfl_xor(bsum[a], 32);
                if (kb0 == 0 && h == 0) db2_part[(long long)part * H2 + n2 + 32 * a] = bs;
            }
        }
    }
}

template <int NB1, int NBH, int HALVES, int S, int V, bool BSUM, int NW = 8>
__global__ __launch_bounds__(NW * 64) void edge_dw2_v3_kernel(
    EdgeGraph g, const __bf16* __restrict__ PQ, int H1, int H2,
    const __bf16* __restrict__ gout, long long ldg, const unsigned char* __restrict__ maskB,
    unsigned char* __restrict__ hbits, float* __restrict__ slab, float* __restrict__ db2_part, int ntiles,
    const unsigned long long* __restrict__ tilevalid)
{
    static_assert(S == 8 || S == 16, "8 or 16 slots per centre");
    constexpr int HP = tr_pitch(NBH * 64);
    constexpr int NLAST = NB1 - (HALVES - 1) * NBH;                // k1 blocks of the last half
    static_assert(NLAST > 0 && NLAST <= NBH, "halves");
    __shared__ __attribute__((aligned(16))) unsigned char Hs[2 * V2_ROWS * HP];
    __shared__ __attribute__((aligned(16))) unsigned char MaskLut[256 * 16];   // byte -> 8 x (0 / 0xFFFF) halfwords
    for (int t = threadIdx.x; t < 256; t += NW * 64) {
        u32x4 e;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
            e[jj] = ((t >> (2 * jj)) & 1 ? 0x0000ffffu : 0u) | ((t >> (2 * jj + 1)) & 1 ? 0xffff0000u : 0u);
        *reinterpret_cast<u32x4*>(&MaskLut[t * 16]) = e;
    }
    __syncthreads();        // the body's prologue reads MaskLut (make_afrag) before its own first barrier
    // The HALVES workgroups of a tile range read the same g_out rows, slot bytes and neighbour ids: place them on the
    // same XCD (blockIdx -> XCD is round-robin over 8) so that the second reader hits that XCD's L2
    const int nparts = ((int)gridDim.x + HALVES - 1) / HALVES;
    int half = (int)blockIdx.x % HALVES, part = (int)blockIdx.x / HALVES;
    if (HALVES == 2 && (nparts & 7) == 0 && (int)gridDim.x == 2 * nparts) {
        const int xcd = (int)blockIdx.x & 7, slot = (int)blockIdx.x >> 3;
        half = slot & 1;
        part = (slot >> 1) * 8 + xcd;
    }
    const unsigned char* PQb = reinterpret_cast<const unsigned char*>(PQ);
    const unsigned char* goutb = reinterpret_cast<const unsigned char*>(gout);
    const unsigned int ldg2 = (unsigned int)ldg * 2u;
    if (NLAST != NBH && half == HALVES - 1)
        edge_dw2_v3_body<NB1, NBH, S, V, NLAST, BSUM, NW>(g, PQb, H1, H2, goutb, ldg2, maskB, hbits, slab, db2_part, ntiles,
                                                               part, nparts, half * NBH, Hs, MaskLut, tilevalid);
    else
        edge_dw2_v3_body<NB1, NBH, S, V, NBH, BSUM, NW>(g, PQb, H1, H2, goutb, ldg2, maskB, hbits, slab, db2_part, ntiles,
                                                             part, nparts, half * NBH, Hs, MaskLut, tilevalid);
}

// =============================================================================== backward (dh, dP, dpre)
// One wave per 32-column block of dh: NB1 = 11 -> an 11-wave (704-thread) workgroup, 3 waves on
// three SIMDs (VGPR budget 168): W2^T slice 64 + accumulators 32 + staging.  NB1 = 4 -> 8 waves.
// The kernel is VALU-bound, so the epilogue is laid out for few instructions per element:
//   * MFMA operands are swapped (W2^T is the "A" operand): a lane holds ONE edge row and 4 consecutive
//     columns per register group -> one h-bit word per row block, bfe + and per element, packed
//     converts, 8-byte LDS writes of the dpre tile;
//   * the slot sums dP[centre] = sum_slots dpre are a second, tiny MFMA: dpre^T (hardware-transposed
//     LDS reads of the wave's own staged block) times a 0/1 slot-selection matrix, instead of 32 adds
//     and cross-lane shuffles per lane.  (dP thus sums the bf16-rounded dpre rows: <= 1.5 bf16 ulp.)
// CP (compact dpre, csrc/dpre_compact.hip): the tile's rows leave the kernel WITHOUT the elements whose h-bit is clear -
// about half the bytes of the tensor that dominated this kernel's HBM writes.  Only the store phase differs: the dense
// tile in `Stage` is compacted in place (every thread first takes its 16-byte chunks into registers, then scatters the
// marked halfwords to their final positions), and the tile goes out as ONE contiguous run at 16 * tilebase[tile].
template <int NB1, int S, int V = 0, bool CP = false>   // H1p = 32 * NB1, H2 == 256, S slots per centre, V: 0 relu / 1 leaky relu (first layer)
__global__ __launch_bounds__((NB1 > 8 ? NB1 : 8) * 64) void edge_bwd_v2_kernel(
    EdgeGraph g, const __bf16* __restrict__ gout, long long ldg, const unsigned char* __restrict__ maskB,
    const unsigned char* __restrict__ hbits, const __bf16* __restrict__ W2Tp,
    __bf16* __restrict__ dpre, __bf16* __restrict__ dP, long long ldp, int ntiles, BwdCompact cp,
    const unsigned long long* __restrict__ tilevalid)
{
    static_assert(!(CP && V != 0), "the leaky variant has no zeros to drop");
    static_assert(S == 8 || S == 16, "8 or 16 slots per centre");
    constexpr int CPT = V2_ROWS / S;               // centres per tile
    constexpr int NT = (NB1 > 8 ? NB1 : 8) * 64;   // threads
    constexpr int K = NB1 * 32;                    // output width (H1p)
    constexpr int K2 = 256, KS2 = K2 / 16;         // contraction (H2)
    constexpr int DP = K2 * 2 + 16;                // dm tile pitch (b128 reads)
    // dpre staging pitch.  The tile is WRITTEN column-wise (swapped operands: the 16 lanes of a ds_write_b64
    // group are 16 consecutive rows at one column, banks (a/4) mod 32) and read back transposed
    // (ds_read_b64_tr_b16: 4 consecutive rows per 32-lane group, banks mod 64).  The transposed-read pitch
    // (== 16 dwords mod 64) puts all 16 rows of a write group on TWO bank pairs: 8-way conflicts, 209M
    // SQ_LDS_BANK_CONFLICT cycles per launch.  A pitch of 18 dwords mod 32 spreads the 16 rows of a write group
    // over all 32 banks (conflict-free) and leaves transposed reads that overlap in 2 banks only; rows are then
    // 8-byte aligned, so the cooperative row reads below are ds_read_b64 pairs instead of ds_read_b128.
    constexpr int SP = stage_pitch(K * 2);
    constexpr int HBW = (V2_ROWS * NB1 + NT - 1) / NT;   // hbits words per thread
    __shared__ __attribute__((aligned(16))) unsigned char Ds[2][V2_ROWS * DP];
    __shared__ __attribute__((aligned(16))) unsigned int Hb[2][V2_ROWS * NB1];
    __shared__ __attribute__((aligned(16))) unsigned char Stage[V2_ROWS * SP];
    __shared__ unsigned short Ro[CP ? 2 : 1][V2_ROWS];          // CP: row starts of the tile (halfwords)
    __shared__ unsigned short WPs[CP ? V2_ROWS * NB1 : 1];      // CP: set bits of a row before each of its words
    // the dump slots of the compact store (2 bytes per thread at the end of Stage) must lie past the largest compact tile
    // (NB1 = 11: up to 43 real chunks per row, i.e. H1 <= 344 - the launcher checks; the reference's 336 has 42)
    static_assert(!CP || V2_ROWS * SP - 2 * NT >= V2_ROWS * 16 * (NB1 == 11 ? 43 : NB1 * 4), "Stage too small for the in-place compaction");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long main_rows = (long long)g.N * S;
    const bool wave_on = wave < NB1;
    const bool builder = wave < 8;                  // waves 0-7 build the dm tile

    // stationary W2^T slice: row n = 32*wave + r of W2Tp [.., K2]
    bf16x8 wa[KS2];
#pragma unroll
    for (int s = 0; s < KS2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) wa[s][e] = (__bf16)0.0f;
    if (wave_on) {
        const __bf16* wrow = W2Tp + (long long)(wave * 32 + r) * K2 + h * 8;
#pragma unroll
        for (int s = 0; s < KS2; ++s) wa[s] = *reinterpret_cast<const bf16x8*>(wrow + s * 16);
    }

    // dm build mapping: lane&31 = 8-column chunk; S = 8: wave = centre, lane>>5 = slot half (4 slots);
    // S = 16: wave>>1 = centre, (wave&1, lane>>5) = slot quarter (4 slots)
    const int bcl = (S == 8) ? (wave & 7) : ((wave & 7) >> 1);
    const int bcc = lane & 31;
    const int bsh = (S == 8) ? (lane >> 5) : (((wave & 1) << 1) | (lane >> 5));
    u32x4 gw = {0u, 0u, 0u, 0u};                    // 8 bf16 of g_out[centre], as stored
    u32x4 mq = {0u, 0u, 0u, 0u};                    // slot masks of those 8 columns: 8 bytes (S=8) / 8 halfwords (S=16)
    unsigned long long tvw = 0ull;                  // V = 2: which rows of the tile exist (edge_fwd_ws_kernel)
    unsigned int hbw[HBW];
    bool dm_ok = false, hb_ok[HBW];
// Loads only ISSUE here (addresses clamped in range); validity masks are applied in GN_V2_WRITE_DM, one
// tile later, so that no s_waitcnt on these loads (and on the dpre stores queued before them) lands at the
// top of the loop.
#define GN_V2_LOAD_DM(tile_)                                                                          \
    {                                                                                                 \
        if (builder) {                                                                                \
            const long long c__ = (long long)(tile_) * CPT + bcl;                                     \
            dm_ok = (tile_) < ntiles && c__ < g.N;                                                    \
            const long long cs__ = dm_ok ? c__ : 0;                                                   \
            if constexpr (V == 2) tvw = tilevalid[(tile_) < ntiles ? (tile_) : 0];                    \
            gw = *reinterpret_cast<const u32x4*>(gout + cs__ * ldg + bcc * 8);                        \
            if constexpr (S == 8) {                                                                   \
                const unsigned int* mp__ = reinterpret_cast<const unsigned int*>(maskB + cs__ * K2 + bcc * 8); \
                mq[0] = mp__[0];                                                                      \
                mq[1] = mp__[1];                                                                      \
            } else {                                                                                  \
                mq = *reinterpret_cast<const u32x4*>(maskB + (cs__ * K2 + bcc * 8) * 2);              \
            }                                                                                         \
        }                                                                                             \
        _Pragma("unroll") for (int i = 0; i < HBW; ++i) {                                             \
            const int w__ = tid + NT * i;                        /* word index in [64][NB1] */        \
            const long long rowg__ = (long long)(tile_) * V2_ROWS + w__ / NB1;                        \
            hb_ok[i] = (tile_) < ntiles && w__ < V2_ROWS * NB1 && rowg__ < main_rows;                 \
            const long long idx__ = hb_ok[i] ? rowg__ * NB1 + (w__ % NB1) : 0;                        \
            hbw[i] = reinterpret_cast<const unsigned int*>(hbits)[idx__];                             \
        }                                                                                             \
    }
#define GN_V2_WRITE_DM(buf_)                                                                          \
    {                                                                                                 \
        if (builder) {                                                                                \
            const u32x4 gw__ = gw;                                                                    \
            const unsigned int okm__ = dm_ok ? (S == 8 ? 0x01010101u : 0x00010001u) : 0u;             \
            u32x4 gs__ = {0u, 0u, 0u, 0u};                       /* V = 2: 0.01 g_out, bf16 */        \
            if constexpr (V == 2) {                                                                   \
                _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {                                    \
                    const unsigned int gj__ = gw__[jj];                                               \
                    gs__[jj] = pack_bf16x2(0.01f * __builtin_bit_cast(float, gj__ << 16),             \
                                           0.01f * __builtin_bit_cast(float, gj__ & 0xffff0000u));    \
                }                                                                                     \
            }                                                                                         \
            _Pragma("unroll") for (int si = 0; si < 4; ++si) {                                        \
                const int slot__ = 4 * bsh + si;                                                      \
                const unsigned int rv__ = (dm_ok && ((tvw >> (S * bcl + slot__)) & 1ull)) ? 0xffffffffu : 0u; \
                u32x4 dw__;                                                                           \
                _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {                                    \
                    unsigned int e__;                            /* {b, 0, b', 0}: bit per bf16 lane */ \
                    if constexpr (S == 8) {                                                           \
                        const unsigned int mw__ = jj < 2 ? mq[0] : mq[1];                             \
                        const unsigned int f__ = (mw__ >> slot__) & okm__;                            \
                        e__ = __builtin_amdgcn_perm(0u, f__, (jj & 1) ? 0x0c030c02u : 0x0c010c00u);   \
                    } else {                                                                          \
                        const unsigned int mw__ = mq[jj];        /* copy the element (no bit_cast) */ \
                        e__ = (mw__ >> slot__) & okm__;                                               \
                    }                                                                                 \
                    const s16x2 mk__ = (s16x2){0, 0} - __builtin_bit_cast(s16x2, e__);                \
                    const unsigned int mku__ = __builtin_bit_cast(unsigned int, mk__);                \
                    if constexpr (V == 2) dw__[jj] = ((gw__[jj] & mku__) | (gs__[jj] & ~mku__)) & rv__;  /* v_bfi_b32 + and */ \
                    else dw__[jj] = gw__[jj] & mku__;                                                 \
                }                                                                                     \
                *reinterpret_cast<u32x4*>(&Ds[buf_][(S * bcl + slot__) * DP + bcc * 16]) = dw__;      \
            }                                                                                         \
        }                                                                                             \
        _Pragma("unroll") for (int i = 0; i < HBW; ++i) {                                             \
            const int w__ = tid + NT * i;                                                             \
            if (w__ < V2_ROWS * NB1) Hb[buf_][w__] = hb_ok[i] ? hbw[i] : 0u;                          \
        }                                                                                             \
    }

    const int per = (ntiles + (int)gridDim.x - 1) / (int)gridDim.x;
    int tile = blockIdx.x * per;
    const int tile_end = min(ntiles, tile + per);
    GN_V2_LOAD_DM(tile);
    GN_V2_WRITE_DM(0);
    if constexpr (CP) { if (tid < V2_ROWS && tile < ntiles) Ro[0][tid] = cp.rowoff[(long long)tile * V2_ROWS + tid]; }
    __syncthreads();

    unsigned int dp_pk[4][2] = {{0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}};
    int buf = 0;
    const int tid_outer = tid;
    const int srow_outer = tid / NB1, sc0_outer = tid % NB1;
    for (; tile < tile_end; ++tile, buf ^= 1) {
        // CP: the thread's coordinates are re-derived per tile from a copy the optimiser cannot trace back to threadIdx,
        // so that NOTHING derived from them (the ~45 per-thread constants of the compact store, but also the LDS / global
        // addresses of the dense part) is hoisted out of the tile loop and parked in registers through the MFMA phase:
        // the kernel sits at the 168-register limit of 11 waves per CU, and every hoisted value was a spill (180 bytes of
        // scratch and 38 reloads per tile in the first build; a kernel of this library may not use scratch at all).
        int tid_l = tid_outer;
        // (V = 2 on the 11-wave shape: the leaky dm build needs the registers too; its row / chunk split - two integer
        // divisions - stays hoisted, the cheap coordinates are re-derived)
        if constexpr (CP || (V == 2 && NB1 > 8)) asm volatile("" : "+v"(tid_l));
        const int tid = tid_l, lane = tid & 63, wave = tid >> 6;
        const int r = lane & 31, h = lane >> 5;
        const bool wave_on = wave < NB1, builder = wave < 8;
        const int bcl = (S == 8) ? (wave & 7) : ((wave & 7) >> 1);
        const int bcc = lane & 31;
        const int bsh = (S == 8) ? (lane >> 5) : (((wave & 1) << 1) | (lane >> 5));
        const int srow = CP ? tid / NB1 : srow_outer, sc0 = CP ? tid % NB1 : sc0_outer;
        GN_V2_LOAD_DM(tile + 1);
        if constexpr (CP) {
            // set bits of a row before each of its h-bit words (Hb[buf] is complete since the last barrier); rows whose
            // slot does not exist keep whatever the dW2 kernel left in their h-bits: they count as empty, like in the plan
            int tid_w = tid;
            asm volatile("" : "+v"(tid_w));               // (not hoisted out of the tile loop: see the store phase)

            if (tid_w < V2_ROWS * NB1) {
                const int srow_w = tid_w / NB1, sc0_w = tid_w % NB1;
                const bool rv = (srow_w % S) < g.K;
                unsigned int run = 0;
                for (int w = 0; w < sc0_w; ++w) run += __builtin_popcount(Hb[buf][srow_w * NB1 + w] & bwd_valid_mask(w, cp.creal));
                WPs[tid_w] = (unsigned short)(rv ? run : 0u);
            }
        }

        if (wave_on) {
            f32x16 a0, a1;                               // row blocks 0 / 1
            zero_acc(a0); zero_acc(a1);
            const unsigned char* p0 = &Ds[buf][r * DP + h * 16];
            const unsigned char* p1 = p0 + 32 * DP;
            const int nb = wave;
            // ---- epilogue pieces: (.) [h > 0] -> dpre tile in LDS; lane = edge row r of the row block,
            //      registers 4g..4g+3 = columns 8g + 4h + (0..3) of this wave's 32-column block
            auto epi_group = [&](const f32x16& acc, int rb, int gq, unsigned int wsh) {
                unsigned char* srow = &Stage[(rb * 32 + r) * SP + (nb * 32 + 4 * h) * 2];
                float d[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float av = acc[4 * gq + j];          // copy the element before any bit_cast
                    const int m = __builtin_amdgcn_sbfe((int)wsh, 8 * gq + j, 1);   // 0 / -1 from bit 8gq+j (v_bfe_i32: one op)
                    if constexpr (V == 0) d[j] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned int, av) & (unsigned int)m);
                    else {
                        // leaky relu (V = 1, 2): slope 1 where h > 0, 0.01 elsewhere: the factor's bits picked by the
                        // 0 / -1 mask (one v_bfi_b32), then one multiply - no compare, no select
                        const unsigned int um = (unsigned int)m;
                        const unsigned int fb = (um & 0x3f800000u) | (~um & 0x3c23d70au);
                        d[j] = av * __builtin_bit_cast(float, fb);
                    }
                }
                typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
                const u32x2_t pk = {pack_bf16x2(d[0], d[1]), pack_bf16x2(d[2], d[3])};
                *reinterpret_cast<u32x2_t*>(srow + 16 * gq) = pk;
            };
            // the chain of row block 0 first; the chain of row block 1 carries the epilogue of block 0 between its
            // MFMAs (one 4-column group every KS2 / 4 steps), so that only block 1's epilogue runs with the matrix pipe idle
#pragma unroll
            for (int s = 0; s < KS2; ++s) {
                const bf16x8 f0 = *reinterpret_cast<const bf16x8*>(p0 + s * 32);
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[s], f0, a0, 0, 0, 0);    // a[n][row]
            }
            const unsigned int wsh0 = Hb[buf][r * NB1 + nb] >> (4 * h);
            const unsigned int wsh1 = Hb[buf][(32 + r) * NB1 + nb] >> (4 * h);
#pragma unroll
            for (int s = 0; s < KS2; ++s) {
                const bf16x8 f1 = *reinterpret_cast<const bf16x8*>(p1 + s * 32);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[s], f1, a1, 0, 0, 0);
                if (s % (KS2 / 4) == 1) epi_group(a0, 0, s / (KS2 / 4), wsh0);
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) epi_group(a1, 1, gq, wsh1);
            // ---- slot sums on the matrix core: dP^T[n][c] = sum_rows dpre[row][n] * [row / 8 == c]
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // own LDS writes before own reads
            f32x16 a2;
            zero_acc(a2);
            {
                typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
                const int g4 = lane >> 4, li = lane & 15;
                const unsigned char* tb = &Stage[(8 * (g4 >> 1) + (li >> 2)) * SP + (16 * (g4 & 1) + 4 * (li & 3)) * 2 + nb * 64];
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tb + (16 * s4) * SP));
                    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tb + (16 * s4 + 4) * SP));
                    const s16x8 dt = __builtin_shufflevector(t0, t1, 0, 1, 2, 3, 4, 5, 6, 7);
                    // rows 16*s4 + 8h .. +7 all belong to ONE centre of the tile: 2*s4 + h (S = 8) or s4 (S = 16)
                    const int cen = (S == 8) ? 2 * s4 + h : s4;
                    const unsigned int one2 = (r == cen) ? 0x3f803f80u : 0u;             // two bf16 ones
                    const u32x4 sel = {one2, one2, one2, one2};
                    a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, dt), __builtin_bit_cast(bf16x8, sel), a2, 0, 0, 0);
                }
            }
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {                           // lane r < CPT holds centre r of the tile
                dp_pk[gq][0] = pack_bf16x2(a2[4 * gq + 0], a2[4 * gq + 1]);
                dp_pk[gq][1] = pack_bf16x2(a2[4 * gq + 2], a2[4 * gq + 3]);
            }
        }
        // The next tile's operands go to LDS BEFORE this tile's dpre stores are issued: vmcnt retires in
        // order, so consuming those loads after the stores would wait for the stores' write acks every tile.
        GN_V2_WRITE_DM(buf ^ 1);
        if (wave_on && r < CPT) {                         // dP rows of the tile's centres (after the prefetch is consumed)
            const long long centre = (long long)tile * (V2_ROWS / S) + r;
            if (centre < g.N) {
                typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const u32x2_t v = {dp_pk[gq][0], dp_pk[gq][1]};
                    *reinterpret_cast<u32x2_t*>(dP + centre * ldp + wave * 32 + 8 * gq + 4 * h) = v;
                }
            }
        }
        __syncthreads();                                  // staging tile + next dm tile complete

        if constexpr (CP) {
            // ---- compact store.  Thread (srow, sc0) owns the 16-byte chunks sc0 + NB1 * i of its row (as below).
            typedef unsigned int u32x2_s __attribute__((ext_vector_type(2)));
            const int tid_c = tid;
            const int tb_cur = cp.tilebase[tile], ts_cur = cp.tilesize16[tile];   // uniform; consumed two barriers from here
            // row starts of the NEXT tile: requested now, parked in LDS at the end of this store phase (no register of
            // the MFMA phase is spent on the prefetch)
            unsigned short ro_next = 0;
            if (tid_c < V2_ROWS) ro_next = cp.rowoff[(long long)(tile + 1 < ntiles ? tile + 1 : tile) * V2_ROWS + tid_c];
            u32x4 val[4];
            unsigned int msk[4], start[4];
            const int srow_c = srow, sc0_c = sc0;       // (per-tile copies: see the top of the loop)
            const bool mine = tid_c < V2_ROWS * NB1;
            if (mine) {
                const long long rowg = (long long)tile * V2_ROWS + srow_c;
                const bool rv = rowg < main_rows && (srow_c % S) < g.K;
                const unsigned int rbase = Ro[buf][srow_c];
                const unsigned char* sp = &Stage[srow_c * SP + sc0_c * 16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int chunk = sc0_c + i * NB1, w = chunk >> 2, b8 = 8 * (chunk & 3);
                    const u32x2_s lo = *reinterpret_cast<const u32x2_s*>(sp + i * NB1 * 16);
                    const u32x2_s hi = *reinterpret_cast<const u32x2_s*>(sp + i * NB1 * 16 + 8);
                    val[i] = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                    const unsigned int word = rv ? (Hb[buf][srow_c * NB1 + w] & bwd_valid_mask(w, cp.creal)) : 0u;
                    msk[i] = (word >> b8) & 0xffu;
                    start[i] = rbase + WPs[srow_c * NB1 + w] + __builtin_popcount(word & ((1u << b8) - 1u));
                }
            }
            __syncthreads();                              // every dense chunk is in registers: Stage may be overwritten
            // the scatter's address arithmetic depends on msk / start only: pinned behind the barrier, or the scheduler
            // computes all 32 (address, value) pairs ahead of it and spills (180 bytes of scratch in the first build)
#pragma unroll
            for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(msk[i]), "+v"(start[i]));
            if (mine) {
                const unsigned int dump = (unsigned int)(V2_ROWS * SP) - 2u * (unsigned int)(tid_c + 1);   // past any compact tile
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    unsigned int cur = 2u * start[i];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const unsigned int bit = (msk[i] >> k) & 1u;
                        const unsigned int dk = val[i][k >> 1];
                        const unsigned short hv = (unsigned short)((k & 1) ? (dk >> 16) : (dk & 0xffffu));
                        *reinterpret_cast<unsigned short*>(&Stage[bit ? cur : dump]) = hv;
                        cur += 2u * bit;
                        if (k & 1) asm volatile("" : "+v"(cur));          // ... and pair by pair inside a chunk
                    }
                }
            }
            __syncthreads();                              // the compact tile is complete
            {
                unsigned char* gp = cp.dpre_c + 16ll * tb_cur;
                for (int idx = tid_c; idx < ts_cur; idx += NT)
                    *reinterpret_cast<u32x4*>(gp + 16ll * idx) = *reinterpret_cast<const u32x4*>(&Stage[16 * idx]);
            }
            if (tid_c < V2_ROWS) Ro[buf ^ 1][tid_c] = ro_next;
        } else
        // cooperative store of the dpre tile: NB1 threads per row, 4 chunks of 16 bytes each at a fixed
        // stride (immediate offsets: one LDS and one global base address per thread, nothing to spill)
        if (tid < V2_ROWS * NB1) {
            const long long rowg = (long long)tile * V2_ROWS + srow;
            if (rowg < main_rows) {
                const unsigned char* sp = &Stage[srow * SP + sc0 * 16];
                unsigned char* gp = reinterpret_cast<unsigned char*>(dpre + rowg * K) + sc0 * 16;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    typedef unsigned int u32x2_s __attribute__((ext_vector_type(2)));
                    const u32x2_s lo = *reinterpret_cast<const u32x2_s*>(sp + i * NB1 * 16);
                    const u32x2_s hi = *reinterpret_cast<const u32x2_s*>(sp + i * NB1 * 16 + 8);
                    *reinterpret_cast<u32x4*>(gp + i * NB1 * 16) = (u32x4){lo[0], lo[1], hi[0], hi[1]};
                }
            }
        }
        __syncthreads();                                  // Stage may be overwritten by the next tile
    }
#undef GN_V2_LOAD_DM
#undef GN_V2_WRITE_DM
}

#undef GN_V2_INFO_ISSUE
#undef GN_V2_INFO
#undef GN_V2_GATHER_WIN

// =============================================================================== launchers (prototypes: edge_v2.hpp)
// One per pass; `variant` (EdgePlan::variant) selects the template argument V.  Each switch below lists every
// instantiation of its kernel that exists.  hipErrorNotSupported = outside the envelope of the variant (edge_plan.hpp).
static inline int v2_tiles(const EdgeGraph& g) { return (int)(((long long)g.N * edge_slots(g.K) + V2_ROWS - 1) / V2_ROWS); }
static bool v2_envelope(int variant, const EdgeGraph& g, int H1p, int H1, int H2) {
    switch (variant) {
        case 0: return edge_v2_shape_ok(g.K, H1p, H2);
        case 1: return edge_v2_max_shape_ok(g.K, H1p, H2) && !g.ovf_cnt;
        case 2: return edge_v2_leaky_shape_ok(g.K, H1p, H1, H2);
        default: return false;
    }
}
// The forward (wave-specialised) and dW2 kernels address P|Q, the output / g_out rows (pitch ld), the slot masks and the
// h-bits with 32-bit offsets and keep node ids in 24 bits.  Forward: rows of `out` in elements (bf16x2 stores), P|Q rows
// in bytes.  N * S * (H1p / 8) < 2^32 (h-bits, tilevalid) follows from the last term: S * (H1p / 8) <= 2 * H1p.
static bool fwd_offsets_ok(const EdgeGraph& g, int H1p, int H2, long long ld) {
    return (long long)g.N * (ld > H2 ? ld : H2) < (1LL << 31) && g.N < (1 << 24) && (long long)g.N * 4 * H1p < (1LL << 32);
}
// dW2: the same set for the pitch of g_out - its byte offsets N * ldg * 2 and N * H2 * 2 below 2^32 ARE the first term
static bool dw2_offsets_ok(const EdgeGraph& g, int H1p, int H2, long long ldg) { return fwd_offsets_ok(g, H1p, H2, ldg); }
// Whether the forward of this layer runs the wave-specialised kernel (launch_edge_fwd_v2 and the plan query of the ABI ask
// here).  Hidden widths 337..352 (all 22 k-steps real) would need 4 more registers for the stationary W2 slice than
// 3 waves per SIMD leave (the variant spilled 24 bytes): the relu variant takes the all-waves-gather kernel for them,
// as it does with GN_EDGE_WS bit 0 clear or offsets beyond 32 bits; the other variants have no such kernel
bool edge_fwd_v2_ws(int variant, const EdgeGraph& g, int H1p, int H1, int H2, long long ldo, const EdgeSwitches& sw) {
    return fwd_offsets_ok(g, H1p, H2, ldo) && (variant != 0 || ((sw.edge_ws & 1) && (H1p == 128 || H1 <= 336)));
}

hipError_t launch_edge_fwd_v2(int variant, const EdgeGraph& g, const void* PQ, int H1p, int H1, const void* W2p, const float* b2,
                              int H2, void* out, long long ldo, float* coords, const CoordCols& cc, unsigned char* maskB,
                              unsigned long long* tilevalid, int num_cus, hipStream_t st) {
    if (!v2_envelope(variant, g, H1p, H1, H2)) return hipErrorNotSupported;
    if (g.N == 0) return hipSuccess;
    const EdgeSwitches sw = edge_switches();
    const bool ws = edge_fwd_v2_ws(variant, g, H1p, H1, H2, ldo, sw);
    if (!ws && variant != 0) return hipErrorNotSupported;
    const int ntiles = v2_tiles(g);
    const int grid = ntiles < num_cus ? ntiles : num_cus;
    const bool s8 = edge_slots(g.K) == 8;
#define GN_FWD_LAUNCH(KS, SS)                                                                              \
    hipLaunchKernelGGL((edge_fwd_v2_kernel<KS, SS>), dim3(grid), dim3(V2_THREADS), 0, st, g, (const __bf16*)PQ,  \
                       (const __bf16*)W2p, b2, H2, (__bf16*)out, ldo, coords, cc, maskB, ntiles)
#define GN_FWD_LAUNCH_WS(KS, KU, SS, V)                                                                    \
    hipLaunchKernelGGL((edge_fwd_ws_kernel<KS, KU, SS, V>), dim3(grid), dim3(WS_THREADS), 0, st, g, (const __bf16*)PQ, \
                       (const __bf16*)W2p, b2, H2, (__bf16*)out, ldo, coords, cc, maskB, ntiles, sw.producers_first, tilevalid)
#define GN_FWD_WS(KS, KU, V) { if (s8) GN_FWD_LAUNCH_WS(KS, KU, 8, V); else GN_FWD_LAUNCH_WS(KS, KU, 16, V); }
    if (!ws) {
        if (H1p == 128) { if (s8) GN_FWD_LAUNCH(8, 8); else GN_FWD_LAUNCH(8, 16); }
        else { if (s8) GN_FWD_LAUNCH(22, 8); else GN_FWD_LAUNCH(22, 16); }
    } else switch (variant) {                    // KSTEPS, KUSE: k-steps of H1p, and those that hold real columns
        case 0: if (H1p == 128) GN_FWD_WS(8, 8, 0) else GN_FWD_WS(22, 21, 0) break;
        case 1: GN_FWD_WS(16, 16, 1) break;
        default: if (H1p == 128) GN_FWD_WS(8, 8, 2) else GN_FWD_WS(22, 21, 2) break;
    }
#undef GN_FWD_LAUNCH
#undef GN_FWD_LAUNCH_WS
#undef GN_FWD_WS
    return hipGetLastError();
}

// number of slabs (= tile-range parts) the dW2 kernel writes for N nodes
int edge_dw2_v2_parts(int N, int K, int H1p, int num_cus) {
    const long long ntiles = ((long long)N * edge_slots(K) + V2_ROWS - 1) / V2_ROWS;
    const int halves = H1p >= 256 ? 2 : 1;
    long long parts = num_cus / halves;
    if (parts > ntiles) parts = ntiles;
    return parts > 0 ? (int)parts : 1;
}

hipError_t launch_edge_dw2_v2(int variant, const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout,
                              long long ldg, const unsigned char* maskB, unsigned char* hbits,
                              const unsigned long long* tilevalid, float* slab, float* db2_part, int num_cus, hipStream_t st) {
    if (!v2_envelope(variant, g, H1p, H1, H2) || !dw2_offsets_ok(g, H1p, H2, ldg)) return hipErrorNotSupported;
    if (g.N == 0) return hipSuccess;
    const int ntiles = v2_tiles(g);
    const int parts = edge_dw2_v2_parts(g.N, g.K, H1p, num_cus);
    const bool s8 = edge_slots(g.K) == 8;
#define GN_DW2_LAUNCH(NB1, NBH, HALVES, SS, V, BSUM)                                                        \
    hipLaunchKernelGGL((edge_dw2_v3_kernel<NB1, NBH, HALVES, SS, V, BSUM>), dim3(parts * HALVES), dim3(V2_THREADS), 0, st, g, \
                       (const __bf16*)PQ, H1, H2, (const __bf16*)gout, ldg, maskB, hbits, slab, db2_part, ntiles, tilevalid)
#define GN_DW2(NB1, NBH, HALVES, V, BSUM) { if (s8) GN_DW2_LAUNCH(NB1, NBH, HALVES, 8, V, BSUM); else GN_DW2_LAUNCH(NB1, NBH, HALVES, 16, V, BSUM); }
    const bool ones = (H1 + 7) / 8 * 8 < H1p;              // a whole pad chunk: db2 comes out of the MFMAs (BSUM = false)
    switch (variant) {
        case 0:
            if (H1p == 128) GN_DW2(4, 4, 1, 0, true) else if (ones) GN_DW2(11, 6, 2, 0, false) else GN_DW2(11, 6, 2, 0, true)
            break;
        case 1: GN_DW2(8, 4, 2, 1, true) break;            // H1 == H1p == 256: no pad chunk
        default: if (H1p == 128) GN_DW2(4, 4, 1, 2, true) else GN_DW2(11, 6, 2, 2, false) break;   // H1 <= 336: a pad chunk
    }
#undef GN_DW2_LAUNCH
#undef GN_DW2
    return hipGetLastError();
}

hipError_t launch_edge_bwd_v2(int variant, const EdgeGraph& g, int H1p, int H2, const void* gout, long long ldg,
                              const unsigned char* maskB, const unsigned char* hbits, const unsigned long long* tilevalid,
                              const void* W2Tp, int H2p, void* dpre, void* dP, long long ldp, int num_cus, hipStream_t st,
                              const BwdCompact* cp) {
    if (!v2_envelope(variant, g, H1p, 0, H2) || H2p != 256 || (cp && variant != 0)) return hipErrorNotSupported;
    if (g.N == 0) return hipSuccess;
    const int ntiles = v2_tiles(g);
    const int grid = ntiles < num_cus ? ntiles : num_cus;
    const bool s8 = edge_slots(g.K) == 8;
    const BwdCompact bc = cp ? *cp : BwdCompact{nullptr, nullptr, nullptr, nullptr, 0};
#define GN_BWD_LAUNCH(NB1, SS, V, CP)                                                                       \
    hipLaunchKernelGGL((edge_bwd_v2_kernel<NB1, SS, V, CP>), dim3(grid), dim3((NB1 > 8 ? NB1 : 8) * 64), 0, st, g, \
                       (const __bf16*)gout, ldg, maskB, hbits, (const __bf16*)W2Tp, (__bf16*)dpre, (__bf16*)dP, ldp, ntiles, bc, tilevalid)
#define GN_BWD(NB1, V, CP) { if (s8) GN_BWD_LAUNCH(NB1, 8, V, CP); else GN_BWD_LAUNCH(NB1, 16, V, CP); }
    switch (variant) {                           // one wave per 32-column block of dh: 512 threads, 704 for H1p = 352
        case 0:
            if (cp) { if (H1p == 128) GN_BWD(4, 0, true) else GN_BWD(11, 0, true) }
            else { if (H1p == 128) GN_BWD(4, 0, false) else GN_BWD(11, 0, false) }
            break;
        case 1: GN_BWD(8, 1, false) break;
        default: if (H1p == 128) GN_BWD(4, 2, false) else GN_BWD(11, 2, false) break;
    }
#undef GN_BWD_LAUNCH
#undef GN_BWD
    return hipGetLastError();
}

}  // namespace gn

