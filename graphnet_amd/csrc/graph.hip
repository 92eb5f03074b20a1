// graphnet_amd/csrc/graph.hip — graph construction kernels over the batched-CSR layout.
//
//   knn_kernel          per-event brute-force k-NN, candidates staged through LDS in chunks,
//                       one query per lane with a register-resident sorted (d2, j) list.
//                       Replaces torch_cluster.knn behind torch_geometric.nn.knn_graph at
//                       models/graphs/edges/edges.py:74-78 and models/components/layers.py:63-67.
//                       With the Minkowski metric (template parameter MT = 1): MinkowskiKNNEdges,
//                       models/graphs/edges/minkowski.py:66-99.
//   radius_*_kernel     per-event radius graph with a neighbour cap (RadialEdges, models/graphs/edges/edges.py:83-117):
//                       in-radius candidates appended in index order; centres above the cap redone with the k-NN list.
//   ovf_*               deterministic compaction of the (k+1)-th "overflow" neighbours.
//   rev_*               reverse adjacency (who gathers from node j) for the backward scatter.
//   globals_kernel      homophily x4 + per-event feature means + log10(n_pulses)
//                       (models/gnn/dynedge.py:266-293, models/utils.py:13-29).
//   scan                exclusive int32 scan used by the compaction / reverse-CSR builders.
//
// HBM-bound integer/byte work: no MFMA here.  Arithmetic that decides k-NN order is kept
// free of FMA contraction so that it is bit-identical to oracle/knn_oracle.c.
#include "common.hpp"

namespace gn {

constexpr int KNN_DMAX = 8;
constexpr int KNN_CH = 256;    // candidates per LDS chunk (8 KB: 20 single-wave workgroups per CU)
constexpr int KNN_TILE = 64;   // queries per workgroup = one wave

struct KnnCols { int c[KNN_DMAX]; };
// Metric of the exhaustive scan (compile time).  0 = squared Euclidean distance (torch_cluster.knn).  1 = the Minkowski
// interval of models/graphs/edges/minkowski.py:10-34,87 with the time-like branch folded in:
//   sp = ((0 + d0*d0) + d1*d1) + ...  over the space columns;  tc = (t_i - t_j) * c;  m = sp - tc*tc;
//   if (m < 0) m = m * (-time_like_weight)
// fp32, operation by operation as oracle/knn_oracle.c:105-146 (no FMA contraction).  The kernel arguments of a metric
// travel in KnnMetric<MT>: nothing for metric 0, whose kernels keep their signature's meaning and their code.
template <int MT> struct KnnMetric {};
template <> struct KnnMetric<1> { int tcol; float c; float ntlw; };      // time column, c, -time_like_weight

// Query tiles are aligned to events: tile t of event e holds queries ptr[e]+64t .. ptr[e]+64t+63, so a
// wave only ever scans candidates of ITS OWN event (a tile spanning events would scan their union).
// tile_ptr[e] = sum_{e'<e} ceil(n_e'/64) is built once per batch by knn_plan_kernel; a workgroup (one
// wave) finds its event by binary search over tile_ptr (wave-uniform scalar loads).
constexpr int KNN_BIG = 256;   // events above this many pulses: candidates split over 8 waves per query tile ...
// ... unless the batch holds so many such tiles that one wave per tile already fills the chip (BASELINE configs[4]:
// 16 events x 10^4 pulses = 2670 tiles on 1024 SIMDs).  A wave that scans its WHOLE event rejects most candidates
// against its running k-th distance with one wave-uniform branch (at 10^4 candidates ~35 % of them still trigger the
// sorted insert for some lane of the wave); a wave that scans one eighth of the event never gets a tight bound
// (nearly every candidate triggers it) and the eight lists must be merged: 2.2x the instructions.  The split only
// pays as a LATENCY measure for a few big events among many small ones.  The choice is made on the device from the
// plan (no host read-back): tile_ptr[B + 1] = number of tiles of big events.
constexpr int KNN_SPLIT_MAX_TILES = 768;
// Candidates that beat a lane's running k-th distance are not inserted at once: the sorted insert is ~4 KMAX vector
// instructions that the WHOLE wave executes even when one lane needs it, and with 64 different queries per wave some
// lane needs it for most candidates (every candidate of a 150-pulse event, ~35 % of them at 10^4 pulses).  Each lane
// appends its (d2, j) to a private FIFO in LDS instead (2 LDS writes); the wave runs the insert sequence once per
// FIFO slot when some lane's FIFO is nearly full: ~ max-over-lanes(inserts) sequences per tile instead of one per
// candidate.  Order is kept (a FIFO per lane, candidates arrive in ascending index), the stale k-th distance only
// admits a few candidates that the real insert then rejects: the lists are the same, entry for entry.
constexpr int KNN_QD = 8;      // FIFO entries per lane; flushed when a lane has more than KNN_QD - 4 (a group adds <= 4)
// Events of thousands of pulses (BASELINE configs[4]: 10^4 per event): the scan is no longer exhaustive.  The event's pulses
// are sorted along a space-filling curve (knn_sort_kernel), every run of 64 sorted pulses gets a bounding box, and a query
// tile (64 consecutive sorted pulses = spatial neighbours) skips every candidate run whose box is farther from all of its
// 64 queries than their running k-th distances (knn_sweep_kernel).  The lists are the same as the exhaustive scan's, entry
// for entry: a skipped candidate fails the (d2, j) test of the list it is kept from (proof at the kernel).
constexpr int KNN_SWEEP_MAX = 16384;     // pulses per event the sort kernel holds in LDS; larger events: exhaustive scan
constexpr int KNN_SWEEP_MIN = 1024;      // events up to this many pulses: exhaustive scan
constexpr int KNN_SWEEP_AVG = 512;       // host side: only batches of >= this many pulses per event launch the two kernels
constexpr int KNN_BOX = 2 * KNN_DMAX;    // floats per bounding box (lo, hi per dimension)
// FIFO depth of the sweep (per lane, in LDS; flushed when a lane holds more than KNN_SQD - 4).  A scanned run is the tile's
// neighbourhood: most of its candidates beat SOME lane's k-th distance and the insert sequence runs for a quarter of them
// whatever the depth - 24 entries measured within 5 % of 8 on four kinds of coordinates, and cost 8 KB more LDS.
constexpr int KNN_SQD = 8;
__device__ __forceinline__ bool knn_sweep_owns(int n, int sweep_min) { return n > sweep_min && n <= KNN_SWEEP_MAX; }
__global__ __launch_bounds__(256) void knn_plan_kernel(const int* __restrict__ ptr, int B, int* __restrict__ tile_ptr) {
    __shared__ int lds[256 / 64];
    int carry = 0;
    for (int e0 = 0; e0 < B; e0 += 256) {
        const int e = e0 + (int)threadIdx.x;
        const int v = e < B ? (max(ptr[e + 1] - ptr[e], 0) + KNN_TILE - 1) / KNN_TILE : 0;
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        if (lane == 63) lds[w] = incl;
        __syncthreads();
        int base = 0, tot = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int sv = lds[i]; if (i < w) base += sv; tot += sv; }
        __syncthreads();
        if (e < B) tile_ptr[e] = carry + base + incl - v;
        carry += tot;
    }
    if (threadIdx.x == 0) { tile_ptr[B] = carry; tile_ptr[B + 1] = 0; }
    __syncthreads();
    // tiles of the events above KNN_BIG pulses (handled by the 8-wave kernel): count at [B+1], ids from [B+2]
    for (int e = threadIdx.x; e < B; e += 256) {
        const int n = max(ptr[e + 1] - ptr[e], 0);
        if (n > KNN_BIG) {
            const int nt = (n + KNN_TILE - 1) / KNN_TILE;
            const int pos = atomicAdd(&tile_ptr[B + 1], nt);
            for (int t = 0; t < nt; ++t) tile_ptr[B + 2 + pos + t] = tile_ptr[e] + t;
        }
    }
}

// DT: number of coordinates at compile time (3 = the usual x,y,z: the distance is 8 instructions), or 0 =
// run-time D <= 8 (every dimension guarded by a select).
// MT: metric (KnnMetric).  MT = 1 stages the time column as one more LDS row (row DM; DT = 0 then holds up to 7 space
// columns), keeps k-entry lists that start at (3.0e38f, -1) - raw times in ns times c reach the Euclidean 1e10f - and drops
// the query BY INDEX where candidates are appended to the FIFO: light-like pairs and coincident pulses sit at m == 0 with
// it, so the "k+1 list with self dropped" argument of metric 0 is not relied on.  A NaN m, or m >= 3.0e38f, never enters.
// Events of ANY size take this exhaustive scan under MT = 1 (both launch shapes, CW = 1 and the 8-wave split): the sorted
// sweep below is not used, its bounding-box bound is a Euclidean lower bound and proves nothing under an indefinite metric.
// CW: waves per query tile.  CW = 1 handles the events with <= KNN_BIG pulses (one wave scans the whole
// event).  CW = 8 handles the larger ones: the candidate range is cut in 8 contiguous pieces, one per wave,
// each wave keeps its own sorted list, and wave 0 merges the 8 lists in ascending piece order with the same
// insertion rule - the result is the same total order (d2, j) as one long scan.  Without it a single
// 5000-pulse event in a batch is a 0.5 ms tail on a 0.13 ms kernel.
template <int KMAX, int DT, int CW, int MT>
__device__ __forceinline__ void knn_tile(
    const int w, unsigned char* lds_raw, unsigned char* lds_queue, const float* __restrict__ x, long long ldx, const KnnCols& cols, int Drt,
    const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N, int k, int strict, int sweep_min,
    int* __restrict__ nbr, int* __restrict__ ovf, const KnnMetric<MT>& mk)
{
#pragma clang fp contract(off)
    constexpr int DM = DT > 0 ? DT : KNN_DMAX - MT;    // (space) dimensions touched by the unrolled loops
    constexpr int DR = DM + MT;                        // staged rows: the time column is row DM
    const int D = DT > 0 ? DT : Drt;
    int elo = 0, ehi = B;                       // largest e with tile_ptr[e] <= w  (empty events share a value)
    while (ehi - elo > 1) {
        const int mid = (elo + ehi) >> 1;
        if (tile_ptr[mid] <= w) elo = mid; else ehi = mid;
    }
    const int ev = elo;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);   // never index past x[N]
    const bool split_big = tile_ptr[B + 1] < KNN_SPLIT_MAX_TILES;         // batch-uniform (see KNN_SPLIT_MAX_TILES)
    if constexpr (MT == 0)
    if (knn_sweep_owns(hi - lo, sweep_min)) return;                // knn_sweep_kernel owns this event
    if ((CW == 1) != (!split_big || hi - lo <= KNN_BIG)) return;   // the other launch owns this event (workgroup-uniform)
    const int kk = MT == 0 ? k + 1 : k;
    const int lane = (int)threadIdx.x & (KNN_TILE - 1), wv = (int)threadIdx.x / KNN_TILE;
    const int q = lo + (w - tile_ptr[ev]) * KNN_TILE + lane;
    const bool active = q < hi;
    float (*cand)[KNN_CH] = reinterpret_cast<float (*)[KNN_CH]>(lds_raw + wv * DR * KNN_CH * 4);   // this wave's staging
    float* qd = reinterpret_cast<float*>(lds_queue) + wv * (2 * KNN_QD * KNN_TILE);               // this wave's FIFOs
    int* qj = reinterpret_cast<int*>(qd + KNN_QD * KNN_TILE);
    int qn = 0;                                                                                   // entries of this lane

    // lanes without a query carry NaN coordinates: every distance is NaN, no comparison holds, nothing is queued
    float qc[DR];
#pragma unroll
    for (int d = 0; d < DM; ++d) qc[d] = d < D ? (active ? x[(long long)q * ldx + cols.c[d]] : __builtin_nanf("")) : 0.0f;
    if constexpr (MT == 1) qc[DM] = active ? x[(long long)q * ldx + mk.tcol] : __builtin_nanf("");
    float bd[KMAX];
    int bj[KMAX];
#pragma unroll
    for (int e = 0; e < KMAX; ++e) { bd[e] = MT == 0 ? 1e10f : 3.0e38f; bj[e] = -1; }

    // sorted insert after equal keys: new[t] = med3(old[t-1], d2, old[t]); the index follows
#define GN_KNN_INSERT(d2_, j_)                                                                        \
    if ((d2_) < bd[KMAX - 1]) {                                                                       \
        bool ct = true;                                   /* d2 < old[t] */                           \
        _Pragma("unroll") for (int t = KMAX - 1; t > 0; --t) {                                        \
            const bool cp = (d2_) < bd[t - 1];            /* d2 < old[t-1] */                         \
            bj[t] = cp ? bj[t - 1] : (ct ? (j_) : bj[t]);                                             \
            bd[t] = __builtin_amdgcn_fmed3f(bd[t - 1], (d2_), bd[t]);                                 \
            ct = cp;                                                                                  \
        }                                                                                             \
        bj[0] = ct ? (j_) : bj[0];                                                                    \
        bd[0] = ct ? (d2_) : bd[0];                                                                   \
    }

#define GN_KNN_FLUSH()                                                                                \
    {                                                                                                 \
        for (int s__ = 0; __ballot(s__ < qn) != 0ull; ++s__) {                                        \
            if (s__ < qn) {                                                                           \
                const float dq__ = qd[s__ * KNN_TILE + lane];                                         \
                const int jq__ = qj[s__ * KNN_TILE + lane];                                           \
                GN_KNN_INSERT(dq__, jq__);                                                            \
            }                                                                                         \
        }                                                                                             \
        qn = 0;                                                                                       \
    }

    // this wave's piece of the candidate range (multiple of 4 long except the last)
    const int piece = CW == 1 ? hi - lo : (((hi - lo + CW - 1) / CW + 3) & ~3);
    const int plo = min(lo + wv * piece, hi), phi = min(plo + piece, hi);
    const int nchunk = (piece + KNN_CH - 1) / KNN_CH;        // same trip count for every wave (barriers inside)
    // The chunk after the one being scanned is already on its way: its loads are issued (into registers) before the scan and
    // land in LDS after it - with 2.6 waves per SIMD (10^4-pulse events) nothing else hid the 40 staging round trips of a tile.
    constexpr int PF = KNN_CH / KNN_TILE;                    // candidates per lane and chunk
    float pre[PF][DR];
    auto prefetch = [&](int ci) {
        const int c0 = plo + ci * KNN_CH;
        const int cn = max(0, min(KNN_CH, phi - c0));
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = lane + u * KNN_TILE;
            const float* row = x + (long long)(c0 + min(t, max(cn - 1, 0))) * ldx;
#pragma unroll
            for (int d = 0; d < DM; ++d) pre[u][d] = (d < D && t < cn) ? row[cols.c[d]] : 3.0e38f;   // pad: d2 = inf, never taken
            if constexpr (MT == 1) pre[u][DM] = t < cn ? row[mk.tcol] : 3.0e38f;     // (metric 1 drops the padding by index)
        }
    };
    if (nchunk > 0) prefetch(0);
    for (int ci = 0; ci < nchunk; ++ci) {
        const int c0 = plo + ci * KNN_CH;
        const int cn = max(0, min(KNN_CH, phi - c0));
        const int cn4 = (cn + 3) & ~3;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = lane + u * KNN_TILE;
            if (t < cn4) {
#pragma unroll
                for (int d = 0; d < DM; ++d)
                    if (d < D) cand[d][t] = pre[u][d];
                if constexpr (MT == 1) cand[DM][t] = pre[u][DM];
            }
        }
        __syncthreads();
        if (ci + 1 < nchunk) prefetch(ci + 1);
        for (int jl = 0; jl < cn4; jl += 4) {
            // Four candidates as two PAIRS per dimension: the float4 read from LDS already holds candidates (u, u + 1) in
            // an aligned register pair, and subtract / square / add on a pair are one packed-fp32 instruction each
            // (v_pk_add_f32 / v_pk_mul_f32: IEEE per element, nothing is fused - the distances are bit for bit the scalar
            // ones).  Left to itself the compiler paired DIMENSIONS of one candidate (x with z, two moves per candidate
            // to assemble the pair): 8 vector instructions per candidate; this is 4.  (No MFMA runs beside this kernel, so
            // the packed-fp32 issue penalty that matters in the edge kernels does not apply.)
            typedef float f32x2_k __attribute__((ext_vector_type(2)));
            f32x2_k d2p[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
            for (int d = 0; d < DM; ++d) {
                if (d < D) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&cand[d][jl]);
                    const f32x2_k q2 = {qc[d], qc[d]};
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        const f32x2_k c2 = {v[2 * pr], v[2 * pr + 1]};
                        const f32x2_k diff = c2 - q2;
                        const f32x2_k sq = diff * diff;
                        d2p[pr] = d2p[pr] + sq;         // 0 + sq first: same left-to-right sum as the oracle
                    }
                }
            }
            if constexpr (MT == 1) {
                // sp -> m, still two packed pairs: subtract, three multiplies (dt*c, its square, the time-like branch),
                // subtract, and one select per candidate.  dt = t_query - t_candidate as the oracle writes it.
                const f32x4 v = *reinterpret_cast<const f32x4*>(&cand[DM][jl]);
                const f32x2_k qt2 = {qc[DM], qc[DM]}, cc2 = {mk.c, mk.c}, nw2 = {mk.ntlw, mk.ntlw};
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {
                    const f32x2_k c2 = {v[2 * pr], v[2 * pr + 1]};
                    const f32x2_k dt = qt2 - c2;
                    const f32x2_k tc = dt * cc2;
                    const f32x2_k tt = tc * tc;
                    const f32x2_k m = d2p[pr] - tt;
                    const f32x2_k mw = m * nw2;
                    d2p[pr][0] = m[0] < 0.0f ? mw[0] : m[0];
                    d2p[pr][1] = m[1] < 0.0f ? mw[1] : m[1];
                }
            }
            // NaN / inf distances (and the NaN of lanes without a query) fail every "<" below.  The query itself is
            // scanned like any other candidate in BOTH modes: strict mode (self excluded, degree <= k) is the
            // k+1-with-self list with the query dropped and cut to k entries - the same k entries, because the
            // query can only be missing from that list when k+1 earlier pulses tie with it at distance 0
            const float d2v[4] = {d2p[0][0], d2p[0][1], d2p[1][0], d2p[1][1]};
            // wave-uniform rejection of the whole group of four against the running k-th distances: in a long scan
            // (thousands of candidates) most groups beat no lane's list.  fmin ignores NaN operands; four NaNs (a lane
            // without a query) compare false.
            const float thr = bd[KMAX - 1];
            const float dmin = __builtin_fminf(__builtin_fminf(d2v[0], d2v[1]), __builtin_fminf(d2v[2], d2v[3]));
            if (__ballot(dmin < thr) != 0ull) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    // metric 1: the query and the padding of the last group are dropped here, by index
                    if (d2v[u] < thr && (MT == 0 || (c0 + jl + u != q && c0 + jl + u < phi))) {
                        qd[qn * KNN_TILE + lane] = d2v[u];
                        qj[qn * KNN_TILE + lane] = c0 + jl + u;
                        ++qn;
                    }
                }
                if (__ballot(qn > KNN_QD - 4) != 0ull) GN_KNN_FLUSH();
            }
        }
    }
    GN_KNN_FLUSH();
    if constexpr (CW > 1) {
        // merge: waves 1.. publish their lists, wave 0 inserts them in ascending piece (= index) order
        __syncthreads();                                    // everybody is done with the staging area
        float* ld = reinterpret_cast<float*>(lds_raw);
        int* lj = reinterpret_cast<int*>(lds_raw) + (CW - 1) * KMAX * KNN_TILE;
        if (wv > 0) {
#pragma unroll
            for (int e = 0; e < KMAX; ++e) {
                ld[((wv - 1) * KMAX + e) * KNN_TILE + lane] = bd[e];
                lj[((wv - 1) * KMAX + e) * KNN_TILE + lane] = bj[e];
            }
        }
        __syncthreads();
        if (wv == 0)
        for (int c = 0; c < CW - 1; ++c)
            for (int e = 0; e < KMAX; ++e) {
                const float d2 = ld[(c * KMAX + e) * KNN_TILE + lane];
                const int j = lj[(c * KMAX + e) * KNN_TILE + lane];
                if (__ballot(d2 < bd[KMAX - 1]) == 0ull) break;          // sorted: nothing further in this list
                GN_KNN_INSERT(d2, j);
            }
    }
    if (active && wv == 0) {
        int c = 0;
        int extra = -1;
#pragma unroll
        for (int e = 0; e < KMAX; ++e) {
            if (e < kk) {
                const int j = bj[e];
                if (j >= 0 && j != q) {
                    if (c < k) nbr[(long long)q * k + c] = j;
                    else if (!strict) extra = j;
                    ++c;
                }
            }
        }
        for (; c < k; ++c) nbr[(long long)q * k + c] = -1;
        if (ovf) ovf[q] = extra;
    }
}

template <int KMAX, int DT, int CW, int MT = 0>
__global__ __launch_bounds__(KNN_TILE * CW) void knn_kernel(
    const float* __restrict__ x, long long ldx, KnnCols cols, int Drt,
    const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N, int k, int strict, int sweep_min,
    int* __restrict__ nbr, int* __restrict__ ovf, KnnMetric<MT> mk)
{
    constexpr int DR = DT > 0 ? DT + MT : KNN_DMAX;     // staged rows (metric 1: the space columns + the time column)
    constexpr int CAND_BYTES = CW * DR * KNN_CH * 4;
    constexpr int LIST_BYTES = (CW - 1) * KMAX * KNN_TILE * 8;
    constexpr int LDS_BYTES = CAND_BYTES > LIST_BYTES ? CAND_BYTES : LIST_BYTES;
    constexpr int QUEUE_BYTES = CW * 2 * KNN_QD * KNN_TILE * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[LDS_BYTES + QUEUE_BYTES];
    unsigned char* lds_raw = lds_all;
    unsigned char* lds_queue = lds_all + LDS_BYTES;
    if constexpr (CW == 1) {
        if ((int)blockIdx.x < tile_ptr[B])
            knn_tile<KMAX, DT, CW, MT>((int)blockIdx.x, lds_raw, lds_queue, x, ldx, cols, Drt, ptr, tile_ptr, B, N, k, strict, sweep_min, nbr, ovf, mk);
    } else {
        const int nbig = tile_ptr[B + 1] < KNN_SPLIT_MAX_TILES ? tile_ptr[B + 1] : 0;   // usually 0: the workgroups leave at once
        for (int i = blockIdx.x; i < nbig; i += gridDim.x) {
            knn_tile<KMAX, DT, CW, MT>(tile_ptr[B + 2 + i], lds_raw, lds_queue, x, ldx, cols, Drt, ptr, tile_ptr, B, N, k, strict, sweep_min, nbr, ovf, mk);
            __syncthreads();                                 // LDS reuse by the next tile
        }
    }
}

// ---------------------------------------------------------------- radius graph (RadialEdges, models/graphs/edges/edges.py:83-117)
// Edge j -> i iff j != i, same event and d2(i, j) < r2 (strict; d2 as in knn_tile: fp32, left to right, no contraction).
// A k-NN list pays ~4 KMAX vector instructions of sorted insert per accepted candidate and a radius graph accepts EVERY
// in-radius candidate, so the common path keeps no list: candidates arrive in ascending index, an in-radius one is stored
// at slot = running count of the centre's row (while the count is below cap) and counted.  A centre that ends at or
// under the cap is finished, already ascending by j.  A tile with a centre above the cap appends its id to a list on the
// device (work[0] = count, ids from work[1]; no host read-back) and radius_overflow_kernel redoes those centres.
//
// radius_scan: the exhaustive scan of one event by one wave, one query per lane - staging, prefetch and the packed-pair
// distance of knn_tile - handing every group of four candidates (j0 .. j0 + 3, d2[4]) to f.  Padding of the last group
// has d2 = inf or NaN and so does everything of a lane without a query (NaN coordinates): no "<" holds for them.
template <int DT, class F>
__device__ __forceinline__ void radius_scan(
    float (*cand)[KNN_CH], const float* __restrict__ x, long long ldx, const KnnCols& cols, int Drt, int lo, int hi, int lane,
    const float (&qc)[DT > 0 ? DT : KNN_DMAX], F&& f)
{
#pragma clang fp contract(off)
    constexpr int DM = DT > 0 ? DT : KNN_DMAX;
    const int D = DT > 0 ? DT : Drt;
    const int nchunk = (hi - lo + KNN_CH - 1) / KNN_CH;
    constexpr int PF = KNN_CH / KNN_TILE;
    float pre[PF][DM];
    auto prefetch = [&](int ci) {
        const int c0 = lo + ci * KNN_CH;
        const int cn = max(0, min(KNN_CH, hi - c0));
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = lane + u * KNN_TILE;
            const float* row = x + (long long)(c0 + min(t, max(cn - 1, 0))) * ldx;
#pragma unroll
            for (int d = 0; d < DM; ++d) pre[u][d] = (d < D && t < cn) ? row[cols.c[d]] : 3.0e38f;   // pad: d2 = inf
        }
    };
    if (nchunk > 0) prefetch(0);
    for (int ci = 0; ci < nchunk; ++ci) {
        const int c0 = lo + ci * KNN_CH;
        const int cn = max(0, min(KNN_CH, hi - c0));
        const int cn4 = (cn + 3) & ~3;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int t = lane + u * KNN_TILE;
            if (t < cn4) {
#pragma unroll
                for (int d = 0; d < DM; ++d)
                    if (d < D) cand[d][t] = pre[u][d];
            }
        }
        __syncthreads();
        if (ci + 1 < nchunk) prefetch(ci + 1);
        for (int jl = 0; jl < cn4; jl += 4) {
            typedef float f32x2_r __attribute__((ext_vector_type(2)));
            f32x2_r d2p[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
            for (int d = 0; d < DM; ++d) {
                if (d < D) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&cand[d][jl]);
                    const f32x2_r q2 = {qc[d], qc[d]};
#pragma unroll
                    for (int pr = 0; pr < 2; ++pr) {
                        const f32x2_r c2 = {v[2 * pr], v[2 * pr + 1]};
                        const f32x2_r diff = c2 - q2;
                        const f32x2_r sq = diff * diff;
                        d2p[pr] = d2p[pr] + sq;         // 0 + sq first: the contract's left-to-right sum
                    }
                }
            }
            const float d2v[4] = {d2p[0][0], d2p[0][1], d2p[1][0], d2p[1][1]};
            f(c0 + jl, d2v);
        }
    }
}

// The event of query tile w and this lane's query: lo / hi = the event's pulse range, q = the query (q >= hi: none).
__device__ __forceinline__ void radius_tile_of(int w, const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N,
                                               int lane, int& lo, int& hi, int& q) {
    int elo = 0, ehi = B;                       // largest e with tile_ptr[e] <= w  (empty events share a value)
    while (ehi - elo > 1) {
        const int mid = (elo + ehi) >> 1;
        if (tile_ptr[mid] <= w) elo = mid; else ehi = mid;
    }
    hi = min(ptr[elo + 1], N); lo = min(max(ptr[elo], 0), hi);            // never index past x[N]
    q = lo + (w - tile_ptr[elo]) * KNN_TILE + lane;
}

// Common path: one wave per query tile, events of any size.  nbr[N, cap] (-1 padded), deg[N] = the UNCAPPED count.
template <int DT>
__global__ __launch_bounds__(KNN_TILE) void radius_append_kernel(
    const float* __restrict__ x, long long ldx, KnnCols cols, int Drt, float r2,
    const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N, int cap,
    int* __restrict__ nbr, int* __restrict__ deg, int* __restrict__ work)
{
    constexpr int DM = DT > 0 ? DT : KNN_DMAX;
    const int D = DT > 0 ? DT : Drt;
    __shared__ __attribute__((aligned(16))) float cand[DM][KNN_CH];
    const int w = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (w >= tile_ptr[B]) return;
    int lo, hi, q;
    radius_tile_of(w, ptr, tile_ptr, B, N, lane, lo, hi, q);
    const bool active = q < hi;
    float qc[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) qc[d] = d < D ? (active ? x[(long long)q * ldx + cols.c[d]] : __builtin_nanf("")) : 0.0f;
    int* const row = nbr + (long long)q * cap;              // touched by lanes with a query only
    int cnt = 0;
    radius_scan<DT>(cand, x, ldx, cols, Drt, lo, hi, lane, qc, [&](int j0, const float (&d2v)[4]) {
        const float dmin = __builtin_fminf(__builtin_fminf(d2v[0], d2v[1]), __builtin_fminf(d2v[2], d2v[3]));
        if (__ballot(dmin < r2) != 0ull) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (d2v[u] < r2 && j0 + u != q && active) {          // the centre is dropped by index
                    if (cnt < cap) row[cnt] = j0 + u;
                    ++cnt;
                }
            }
        }
    });
    if (active) {
        for (int c = cnt; c < cap; ++c) row[c] = -1;
        deg[q] = cnt;
    }
    if (__ballot(active && cnt > cap) != 0ull && lane == 0) work[1 + atomicAdd(&work[0], 1)] = w;
}

// Rare path: the tiles listed in work, a few workgroups striding over them.  Every centre of such a tile above the cap
// keeps a register-resident sorted (d2, j) list as knn_tile does (FIFO and insert are knn_tile's), started at (r2, -1) so
// that only in-radius candidates enter, the centre dropped by index.  Its cap-th entry (td, tj) is the largest kept key:
// a second scan stores every in-radius j with (d2, j) <= (td, tj) - exactly cap of them, the distances are the same bits -
// in ascending j, which is the order the table wants and costs no sort of the list.
template <int KMAX, int DT>
__global__ __launch_bounds__(KNN_TILE) void radius_overflow_kernel(
    const float* __restrict__ x, long long ldx, KnnCols cols, int Drt, float r2,
    const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N, int cap,
    int* __restrict__ nbr, const int* __restrict__ deg, const int* __restrict__ work)
{
    constexpr int DM = DT > 0 ? DT : KNN_DMAX;
    const int D = DT > 0 ? DT : Drt;
    __shared__ __attribute__((aligned(16))) float cand[DM][KNN_CH];
    __shared__ float qd[KNN_QD * KNN_TILE];
    __shared__ int qj[KNN_QD * KNN_TILE];
    const int lane = (int)threadIdx.x;
    const int ntile = min(work[0], tile_ptr[B]);
    for (int i = (int)blockIdx.x; i < ntile; i += (int)gridDim.x) {
        const int w = work[1 + i];
        int lo, hi, q;
        radius_tile_of(w, ptr, tile_ptr, B, N, lane, lo, hi, q);
        const bool over = q < hi && deg[q] > cap;           // the others are finished (and scan as lanes without a query)
        float qc[DM];
#pragma unroll
        for (int d = 0; d < DM; ++d) qc[d] = d < D ? (over ? x[(long long)q * ldx + cols.c[d]] : __builtin_nanf("")) : 0.0f;
        float bd[KMAX];
        int bj[KMAX];
#pragma unroll
        for (int e = 0; e < KMAX; ++e) { bd[e] = r2; bj[e] = -1; }
        int qn = 0;
        radius_scan<DT>(cand, x, ldx, cols, Drt, lo, hi, lane, qc, [&](int j0, const float (&d2v)[4]) {
            const float thr = bd[KMAX - 1];
            const float dmin = __builtin_fminf(__builtin_fminf(d2v[0], d2v[1]), __builtin_fminf(d2v[2], d2v[3]));
            if (__ballot(dmin < thr) != 0ull) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (d2v[u] < thr && j0 + u != q) {
                        qd[qn * KNN_TILE + lane] = d2v[u];
                        qj[qn * KNN_TILE + lane] = j0 + u;
                        ++qn;
                    }
                }
                if (__ballot(qn > KNN_QD - 4) != 0ull) GN_KNN_FLUSH();
            }
        });
        GN_KNN_FLUSH();
        float td = -1.0f;                                   // lanes that are not over keep nothing (d2 >= 0)
        int tj = -1;
#pragma unroll
        for (int e = 0; e < KMAX; ++e)
            if (e == cap - 1 && over) { td = bd[e]; tj = bj[e]; }
        int* const row = nbr + (long long)q * cap;          // touched by lanes that are over only
        int cnt = 0;
        radius_scan<DT>(cand, x, ldx, cols, Drt, lo, hi, lane, qc, [&](int j0, const float (&d2v)[4]) {
            const float dmin = __builtin_fminf(__builtin_fminf(d2v[0], d2v[1]), __builtin_fminf(d2v[2], d2v[3]));
            if (__ballot(dmin <= td) != 0ull) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = j0 + u;
                    if ((d2v[u] < td || (d2v[u] == td && j <= tj)) && j != q && cnt < cap) row[cnt++] = j;
                }
            }
        });
    }
}
#undef GN_KNN_INSERT
#undef GN_KNN_FLUSH

// ---------------------------------------------------------------- k-NN of large events: sort + pruned sweep
// One workgroup per event that the sweep owns.  Key = 18-bit Morton code of the first (up to) three coordinates, quantised
// to 6 bits inside the event's box of finite values, then the pulse's position in the event (14 bits): keys are distinct,
// the order is deterministic.  ANY order gives the right lists - the order only decides how much the sweep can skip.
// Out: sidx[ptr[e] + p] = global index of the p-th sorted pulse, sx[d][ptr[e] + p] = its coordinates (dimension-major: the
// sweep's loads are contiguous), bbox[tile][2d], [2d + 1] = min / max of coordinate d over the 64 pulses of a run (NaN
// coordinates left out: such a candidate is never a neighbour), tile = tile_ptr[e] + p / 64.
template <int DT>
__global__ __launch_bounds__(1024) void knn_sort_kernel(
    const float* __restrict__ x, long long ldx, KnnCols cols, int Drt, const int* __restrict__ ptr, const int* __restrict__ tile_ptr,
    int B, int N, int sweep_min, int* __restrict__ sidx, float* __restrict__ sx, float* __restrict__ bbox, int* __restrict__ bminj)
{
    constexpr int DM = DT > 0 ? DT : KNN_DMAX;
    const int D = DT > 0 ? DT : Drt;
    __shared__ unsigned int skey[KNN_SWEEP_MAX];
    __shared__ float red[2][3][16];
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int n = hi - lo;
    if (!knn_sweep_owns(n, sweep_min)) return;
    const int MD = D < 3 ? D : 3;
    const float inf = __builtin_inff();
    float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    for (int i = tid; i < n; i += 1024) {
        const float* row = x + (long long)(lo + i) * ldx;
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < MD) {
                const float v = row[cols.c[d]];
                if (__builtin_fabsf(v) < inf) { mn[d] = __builtin_fminf(mn[d], v); mx[d] = __builtin_fmaxf(mx[d], v); }
            }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[d] = __builtin_fminf(mn[d], __shfl_xor(mn[d], o));
            mx[d] = __builtin_fmaxf(mx[d], __shfl_xor(mx[d], o));
        }
        if (lane == 0) { red[0][d][wv] = mn[d]; red[1][d][wv] = mx[d]; }
    }
    __syncthreads();
    float scale[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        float a = inf, b = -inf;
#pragma unroll
        for (int i = 0; i < 16; ++i) { a = __builtin_fminf(a, red[0][d][i]); b = __builtin_fmaxf(b, red[1][d][i]); }
        mn[d] = a;
        scale[d] = b > a ? 64.0f / (b - a) : 0.0f;
    }
    int P = 64;
    while (P < n) P <<= 1;
    for (int i = tid; i < P; i += 1024) {
        unsigned int key = 0xffffffffu;
        if (i < n) {
            const float* row = x + (long long)(lo + i) * ldx;
            unsigned int code = 0;
#pragma unroll
            for (int d = 0; d < 3; ++d)
                if (d < MD) {
                    const float f = (row[cols.c[d]] - mn[d]) * scale[d];
                    const unsigned int q = f >= 0.0f ? (f < 63.0f ? (unsigned int)f : 63u) : 0u;      // NaN -> 0
                    const unsigned int sp = (q & 1u) | ((q & 2u) << 2) | ((q & 4u) << 4) | ((q & 8u) << 6) | ((q & 16u) << 8) | ((q & 32u) << 10);
                    code |= sp << d;
                }
            key = (code << 14) | (unsigned int)i;
        }
        skey[i] = key;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 1024) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned int a = skey[i], b = skey[l];
                if ((a > b) == ((i & kk) == 0)) { skey[i] = b; skey[l] = a; }
            }
            __syncthreads();
        }
    const int nr = (n + 63) & ~63;                       // whole waves: a wave's 64 lanes are one run
    const long long tile0 = tile_ptr[ev];
    for (int i = tid; i < nr; i += 1024) {
        const bool valid = i < n;
        const int src = lo + (valid ? (int)(skey[i] & 16383u) : 0);
        if (valid) sidx[lo + i] = src;
        int mj = valid ? src : 0x7fffffff;                  // smallest pulse index of the run
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mj = min(mj, __shfl_xor(mj, o));
        if (lane == 0) bminj[tile0 + (i >> 6)] = mj;
#pragma unroll
        for (int d = 0; d < DM; ++d)
            if (d < D) {
                const float v = x[(long long)src * ldx + cols.c[d]];
                if (valid) sx[(long long)d * N + lo + i] = v;
                float a = (valid && v == v) ? v : inf, b = (valid && v == v) ? v : -inf;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    a = __builtin_fminf(a, __shfl_xor(a, o));
                    b = __builtin_fmaxf(b, __shfl_xor(b, o));
                }
                if (lane == 0) {
                    bbox[(tile0 + (i >> 6)) * KNN_BOX + 2 * d] = a;
                    bbox[(tile0 + (i >> 6)) * KNN_BOX + 2 * d + 1] = b;
                }
            }
    }
}

// One wave per query tile = run t of the sorted event, one query per lane, lists in registers (as knn_tile).
// A candidate run c is skipped when, for every query of the tile, (lb, min_j) >= (thr, j_last): lb = the distance formula
// applied to the per-dimension gaps between the query and the run's box, min_j = the smallest pulse index of the run,
// (thr, j_last) = the query's running k-th entry.  Exactness: for a candidate of the run and each dimension
// |c_d - q_d| >= gap_d; rounding is monotone, so fl((c_d - q_d)^2) >= fl(gap_d^2) and the left-to-right fp32 sum d2 >= lb;
// its index j >= min_j; so (d2, j) >= (lb, min_j) >= the list's last entry, which only ever decreases.
// Candidates arrive out of index order here, so the lists hold 64-bit keys - bits of d2 (a sum of squares: non-negative,
// the bit pattern orders like the value; NaN and inf sort above the 1e10 sentinel and never enter), then the pulse index:
// (d2, j) < (d2', j') is one v_cmp_lt_u64, keys are distinct, and the list is the (d2, j)-sorted list that the
// ascending-index scan of knn_tile builds, whatever the order of arrival.  The insert is branch-free, 5 instructions per
// list position (the lexicographic compare on separate registers compiled to a chain of exec-mask branches: 2000 cycles
// per insert sequence, measured with s_memtime; this form: 1270 beside two other waves).
template <int KMAX, int DT>
__global__ __launch_bounds__(KNN_TILE) void knn_sweep_kernel(
    int Drt, const int* __restrict__ ptr, const int* __restrict__ tile_ptr, int B, int N, int k, int strict, int sweep_min,
    const int* __restrict__ sidx, const float* __restrict__ sx, const float* __restrict__ bbox, const int* __restrict__ bminj,
    int* __restrict__ nbr, int* __restrict__ ovf)
{
#pragma clang fp contract(off)
    constexpr int DM = DT > 0 ? DT : KNN_DMAX;
    const int D = DT > 0 ? DT : Drt;
    typedef unsigned long long u64;
    typedef float f32x2_k __attribute__((ext_vector_type(2)));
    typedef int i32x4_k __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float cand[DM][KNN_TILE];
    __shared__ __attribute__((aligned(16))) int cj[KNN_TILE];
    __shared__ float qd[KNN_SQD * KNN_TILE];
    __shared__ int qj[KNN_SQD * KNN_TILE];
    const int w = (int)blockIdx.x;
    if (w >= tile_ptr[B]) return;
    int elo = 0, ehi = B;
    while (ehi - elo > 1) {
        const int mid = (elo + ehi) >> 1;
        if (tile_ptr[mid] <= w) elo = mid; else ehi = mid;
    }
    const int ev = elo;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    if (!knn_sweep_owns(hi - lo, sweep_min)) return;
    const int tile0 = tile_ptr[ev];
    const int t = w - tile0, nch = (hi - lo + KNN_TILE - 1) / KNN_TILE;
    const int lane = (int)threadIdx.x;
    const int pos = lo + t * KNN_TILE + lane;
    const bool active = pos < hi;
    const int q = active ? sidx[pos] : -1;
    const int kk = k + 1;
    float qc[DM];
    bool live = active;                              // a query with a NaN coordinate takes nothing: it never keeps a run alive
#pragma unroll
    for (int d = 0; d < DM; ++d) {
        qc[d] = d < D ? (active ? sx[(long long)d * N + pos] : __builtin_nanf("")) : 0.0f;
        live = live && qc[d] == qc[d];
    }
    constexpr u64 EMPTY = (u64)0x501502f9u << 32;        // (1e10f, 0): no candidate's key is below its own distance's 1e10
    u64 bk[KMAX];
#pragma unroll
    for (int e = 0; e < KMAX; ++e) bk[e] = EMPTY;
    int qn = 0;
#define GN_KNN_KEY(d_, j_) (((u64)__builtin_bit_cast(unsigned int, (d_)) << 32) | (unsigned int)(j_))
#define GN_KNN_THR() __builtin_bit_cast(float, (unsigned int)(bk[KMAX - 1] >> 32))
#define GN_KNN_INSERT2(key_)                                                                          \
    {                                                                                                 \
        bool ct = (key_) < bk[KMAX - 1];                                                              \
        _Pragma("unroll") for (int t_ = KMAX - 1; t_ > 0; --t_) {                                     \
            const bool cp = (key_) < bk[t_ - 1];                                                      \
            bk[t_] = cp ? bk[t_ - 1] : (ct ? (key_) : bk[t_]);                                        \
            ct = cp;                                                                                  \
        }                                                                                             \
        bk[0] = ct ? (key_) : bk[0];                                                                  \
    }
#define GN_KNN_FLUSH2()                                                                               \
    {                                                                                                 \
        for (int s__ = 0; __ballot(s__ < qn) != 0ull; ++s__) {                                        \
            const float dq__ = qd[s__ * KNN_TILE + lane];                                             \
            const int jq__ = qj[s__ * KNN_TILE + lane];                                               \
            const u64 kq__ = s__ < qn ? GN_KNN_KEY(dq__, jq__) : ~0ull;                               \
            GN_KNN_INSERT2(kq__);                                                                     \
        }                                                                                             \
        qn = 0;                                                                                       \
    }
    // scan of one candidate run (wave-uniform c_)
#define GN_KNN_SCAN_RUN(c_)                                                                           \
    {                                                                                                 \
        __syncthreads();                                                                              \
        const int cpos = lo + (c_) * KNN_TILE + lane;                                                 \
        const bool cv = cpos < hi;                                                                    \
        _Pragma("unroll") for (int d = 0; d < DM; ++d)                                                \
            if (d < D) cand[d][lane] = cv ? sx[(long long)d * N + cpos] : 3.0e38f;   /* pad: d2 = inf */ \
        cj[lane] = cv ? sidx[cpos] : 0x7fffffff;                                                      \
        __syncthreads();                                                                              \
        for (int jl = 0; jl < KNN_TILE; jl += 4) {                                                    \
            f32x2_k d2p[2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};                                            \
            _Pragma("unroll") for (int d = 0; d < DM; ++d) {                                          \
                if (d < D) {                                                                          \
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&cand[d][jl]);                    \
                    const f32x2_k q2 = {qc[d], qc[d]};                                                \
                    _Pragma("unroll") for (int pr = 0; pr < 2; ++pr) {                                \
                        const f32x2_k c2 = {v[2 * pr], v[2 * pr + 1]};                                \
                        const f32x2_k diff = c2 - q2;                                                 \
                        const f32x2_k sq = diff * diff;                                               \
                        d2p[pr] = d2p[pr] + sq;      /* 0 + sq first: the oracle's left-to-right sum */ \
                    }                                                                                 \
                }                                                                                     \
            }                                                                                         \
            const float d2v[4] = {d2p[0][0], d2p[0][1], d2p[1][0], d2p[1][1]};                        \
            const u64 klast = bk[KMAX - 1];                                                           \
            const float thr = GN_KNN_THR();                                                           \
            const float dmin = __builtin_fminf(__builtin_fminf(d2v[0], d2v[1]), __builtin_fminf(d2v[2], d2v[3])); \
            if (__ballot(dmin <= thr) != 0ull) {                                                      \
                const i32x4_k jv = *reinterpret_cast<const i32x4_k*>(&cj[jl]);                        \
                _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                       \
                    if (GN_KNN_KEY(d2v[u], jv[u]) < klast) {                                          \
                        qd[qn * KNN_TILE + lane] = d2v[u];                                            \
                        qj[qn * KNN_TILE + lane] = jv[u];                                             \
                        ++qn;                                                                         \
                    }                                                                                 \
                }                                                                                     \
                if (__ballot(qn > KNN_SQD - 4) != 0ull) GN_KNN_FLUSH2();                              \
            }                                                                                         \
        }                                                                                             \
    }

    // Visiting order: the tile's own run first (64 spatial neighbours: a first bound), then the other runs by ascending
    // box-to-box distance from the tile (ties: ascending run index), until the nearest unvisited box is farther than the
    // tile's largest k-th distance.  Inside a group of coincident pulses (a DOM's pulses: ties at distance 0) the boxes tie
    // at 0 and the sorted order is the index order: after the group's first run holds the list's k+1 smallest indices every
    // later run of the group fails the index test as a whole - a descending visit would insert every candidate of the group.
    GN_KNN_SCAN_RUN(t);
    GN_KNN_FLUSH2();                                      // the first real k-th distances
    // the tile's own box (all live queries are inside it): box-to-box gaps bound the per-query gaps from below
    float qlo[DM], qhi[DM];
#pragma unroll
    for (int d = 0; d < DM; ++d) {
        qlo[d] = d < D ? bbox[(long long)(tile0 + t) * KNN_BOX + 2 * d] : 0.0f;
        qhi[d] = d < D ? bbox[(long long)(tile0 + t) * KNN_BOX + 2 * d + 1] : 0.0f;
    }
    // lane l keeps the box distances of runs l, 64 + l, 128 + l, 192 + l (KNN_SWEEP_MAX / 64 = 256 runs at most) as sort keys:
    // bits of the (non-negative) distance, then the run index; ~0 = visited / absent
    constexpr int NBLK = KNN_SWEEP_MAX / KNN_TILE / KNN_TILE;
    constexpr bool BOXREG = DT > 0 && DT <= 4;          // the boxes stay in registers: the per-query test reads them with
    constexpr int BR = BOXREG ? DM : 1;                 // v_readlane instead of a dependent load per visited run
    u64 key[NBLK];
    float rlo[NBLK][BR], rhi[NBLK][BR];
    int rmj[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        const int cl = b * KNN_TILE + lane;
        key[b] = ~0ull;
        rmj[b] = 0;
#pragma unroll
        for (int d = 0; d < BR; ++d) { rlo[b][d] = 0.0f; rhi[b][d] = 0.0f; }
        if (cl < nch && cl != t) {
            const float* bb = bbox + (long long)(tile0 + cl) * KNN_BOX;
            float lbb = 0.0f;
#pragma unroll
            for (int d = 0; d < DM; ++d)
                if (d < D) {
                    const float l0 = bb[2 * d], h0 = bb[2 * d + 1];
                    if constexpr (BOXREG) { rlo[b][d] = l0; rhi[b][d] = h0; }
                    const float gap = __builtin_fmaxf(__builtin_fmaxf(l0 - qhi[d], qlo[d] - h0), 0.0f);
                    const float sq = gap * gap;
                    lbb = lbb + sq;
                }
            if constexpr (BOXREG) rmj[b] = bminj[tile0 + cl];
            key[b] = ((u64)__builtin_bit_cast(unsigned int, lbb) << 32) | (unsigned int)cl;
        }
    }
    for (;;) {
        u64 best = key[0];
#pragma unroll
        for (int b = 1; b < NBLK; ++b) best = key[b] < best ? key[b] : best;
        float tmax = live ? GN_KNN_THR() : -1.0f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned int olo = __shfl_xor((unsigned int)best, o), ohi = __shfl_xor((unsigned int)(best >> 32), o);
            const u64 other = ((u64)ohi << 32) | olo;
            best = other < best ? other : best;
            tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, o));
        }
        if (best == ~0ull) break;
        const float lbmin = __builtin_bit_cast(float, (unsigned int)(best >> 32));
        if (lbmin > tmax) break;                             // every unvisited box is at least this far
        const int c = __builtin_amdgcn_readfirstlane((int)(unsigned int)best);
#pragma unroll
        for (int b = 0; b < NBLK; ++b)
            if (c == b * KNN_TILE + lane) key[b] = ~0ull;
        // per-query test against the run's box
        float bl[DM], bh[DM];
        int mj = 0;
        if constexpr (BOXREG) {
            const int src = c & (KNN_TILE - 1);
#pragma unroll
            for (int b = 0; b < NBLK; ++b)
                if ((c >> 6) == b) {                         // wave-uniform
#pragma unroll
                    for (int d = 0; d < DM; ++d) {
                        bl[d] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rlo[b][d]), src));
                        bh[d] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rhi[b][d]), src));
                    }
                    mj = __builtin_amdgcn_readlane(rmj[b], src);
                }
        } else {
            const float* bb = bbox + (long long)(tile0 + c) * KNN_BOX;
#pragma unroll
            for (int d = 0; d < DM; ++d) { bl[d] = d < D ? bb[2 * d] : 0.0f; bh[d] = d < D ? bb[2 * d + 1] : 0.0f; }
            mj = bminj[tile0 + c];
        }
        float lb = 0.0f;
#pragma unroll
        for (int d = 0; d < DM; ++d)
            if (d < D) {
                const float gap = __builtin_fmaxf(__builtin_fmaxf(bl[d] - qc[d], qc[d] - bh[d]), 0.0f);
                const float sq = gap * gap;
                lb = lb + sq;
            }
        // a candidate of the run has d2 >= lb and j >= mj: it cannot enter a list whose last entry is not above (lb, mj)
        if (__ballot(live && GN_KNN_KEY(lb, mj) < bk[KMAX - 1]) == 0ull) continue;
        GN_KNN_SCAN_RUN(c);
    }
    GN_KNN_FLUSH2();
#undef GN_KNN_SCAN_RUN
#undef GN_KNN_FLUSH2
#undef GN_KNN_INSERT2
#undef GN_KNN_KEY
#undef GN_KNN_THR
    if (active) {
        int c = 0;
        int extra = -1;
#pragma unroll
        for (int e = 0; e < KMAX; ++e) {
            if (e < kk) {
                const int j = bk[e] == EMPTY ? -1 : (int)(unsigned int)bk[e];
                if (j >= 0 && j != q) {
                    if (c < k) nbr[(long long)q * k + c] = j;
                    else if (!strict) extra = j;
                    ++c;
                }
            }
        }
        for (; c < k; ++c) nbr[(long long)q * k + c] = -1;
        if (ovf) ovf[q] = extra;
    }
}

// ---------------------------------------------------------------- exclusive scan (int32)
constexpr int SCAN_BLOCK = 256;
constexpr int SCAN_ITEMS = 8;   // per thread -> 2048 per block

__device__ __forceinline__ int block_exclusive_scan(int v, int* total, int* lds) {
    // lds: SCAN_BLOCK/64 ints
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SCAN_BLOCK / 64; ++i) {
        const int s = lds[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - v;
}

// FLAG: scan the predicate (in[i] >= 0) instead of in[i] (stream compaction without a separate flag pass)
template <bool FLAG>
__global__ __launch_bounds__(SCAN_BLOCK) void scan_phase1(const int* __restrict__ in, int n,
                                                          int* __restrict__ out, int* __restrict__ bsum, int* __restrict__ total_out) {
    __shared__ int lds[SCAN_BLOCK / 64];
    const int base = (blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_ITEMS;
    int v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        const int x = (base + i < n) ? in[base + i] : (FLAG ? -1 : 0);
        v[i] = FLAG ? (x >= 0 ? 1 : 0) : x;
        s += v[i];
    }
    int tot;
    int ex = block_exclusive_scan(s, &tot, lds);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) { if (base + i < n) out[base + i] = ex; ex += v[i]; }
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = tot;
        if (total_out) *total_out = tot;                 // single-block scan (n <= 2048): this launch is the whole scan
    }
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_phase2(int* __restrict__ bsum, int nb, int* __restrict__ total_out) {
    __shared__ int lds[SCAN_BLOCK / 64];
    int carry = 0;
    for (int c0 = 0; c0 < nb; c0 += SCAN_BLOCK) {
        const int i = c0 + threadIdx.x;
        const int v = (i < nb) ? bsum[i] : 0;
        int tot;
        const int ex = block_exclusive_scan(v, &tot, lds);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

__global__ __launch_bounds__(SCAN_BLOCK) void scan_phase3(int* __restrict__ out, int n, const int* __restrict__ bsum) {
    const int base = (blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_ITEMS;
    const int add = bsum[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) if (base + i < n) out[base + i] += add;
}
// phases 2 + 3 in one launch (few blocks): every block sums the RAW block totals before it by itself
__global__ __launch_bounds__(SCAN_BLOCK) void scan_phase23(int* __restrict__ out, int n, const int* __restrict__ bsum,
                                                           int* __restrict__ total_out) {
    __shared__ int lds[SCAN_BLOCK / 64];
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += SCAN_BLOCK) part += bsum[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = part;
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int i = 0; i < SCAN_BLOCK / 64; ++i) add += lds[i];
    const int base = (blockIdx.x * SCAN_BLOCK + threadIdx.x) * SCAN_ITEMS;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) if (base + i < n) out[base + i] += add;
    if (total_out && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total_out = add + bsum[blockIdx.x];
}

// ---------------------------------------------------------------- overflow compaction
__global__ __launch_bounds__(256) void flag_nonneg(const int* __restrict__ v, int n, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = v[i] >= 0 ? 1 : 0;
}
// pos = exclusive scan of flags; writes centre ids (ascending) and their overflow sources
__global__ __launch_bounds__(256) void ovf_write(const int* __restrict__ ovf, const int* __restrict__ pos, int n,
                                                 int* __restrict__ ovf_centre, int* __restrict__ ovf_src) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && ovf[i] >= 0) { ovf_centre[pos[i]] = i; ovf_src[pos[i]] = ovf[i]; }
}

// ---------------------------------------------------------------- reverse adjacency
// rows: r = i*S + slot for the fixed-stride table (S slots per centre), r = N*S + t for
// overflow edge t.  cnt[j] += 1 for each row whose source is j.
__global__ __launch_bounds__(256) void rev_count(const int* __restrict__ nbr, int N, int K, int S,
                                                 const int* __restrict__ ovf_src, const int* __restrict__ ovf_cnt,
                                                 int* __restrict__ cnt) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long main_rows = (long long)N * S;
    if (t < main_rows) {
        const int i = (int)(t / S), s = (int)(t % S);
        if (s < K) { const int j = nbr[(long long)i * K + s]; if (j >= 0) atomicAdd(&cnt[j], 1); }
    } else if (ovf_cnt && t - main_rows < *ovf_cnt) {
        atomicAdd(&cnt[ovf_src[t - main_rows]], 1);
    }
}
__global__ __launch_bounds__(256) void rev_fill(const int* __restrict__ nbr, int N, int K, int S,
                                                const int* __restrict__ ovf_src, const int* __restrict__ ovf_cnt,
                                                const int* __restrict__ rev_ptr, int* __restrict__ cursor,
                                                int* __restrict__ rev_rows, int* __restrict__ hub_count) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long main_rows = (long long)N * S;
    int j = -1;
    if (t < main_rows) {
        const int i = (int)(t / S), s = (int)(t % S);
        if (s < K) j = nbr[(long long)i * K + s];
    } else if (ovf_cnt && t - main_rows < *ovf_cnt) {
        j = ovf_src[t - main_rows];
    }
    if (j >= 0) {
        const int p = atomicSub(&cursor[j], 1) - 1;      // cursor[j] = in-degree left to place: counts down to 0
        rev_rows[rev_ptr[j] + p] = (int)t;
    }
    if (t == 0) *hub_count = 0;                          // reset for rev_find_hubs (next kernel)
}

// The in-edge lists are filled with atomics (arbitrary order).  The dQ gather sums rows in ascending row
// id (fixed order -> reproducible): lists of <= 64 entries are ordered by the gathering wave itself, longer
// ones (hub pulses: many pulses on one DOM share coordinates, so the lowest-index ones are everybody's
// neighbours) are sorted here once per graph, in LDS, one workgroup per hub node.
constexpr int REV_SORT_MIN = 64;          // lists longer than this are sorted by rev_sort_kernel
constexpr int REV_SORT_CAP = 16384;       // ... up to this many entries (64 KB of LDS)
__global__ __launch_bounds__(256) void rev_find_hubs(const int* __restrict__ rev_ptr, int N, int* __restrict__ hubs,
                                                     int* __restrict__ nhubs) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= N) return;
    const int d = rev_ptr[j + 1] - rev_ptr[j];
    if (d > REV_SORT_MIN && d <= REV_SORT_CAP) hubs[atomicAdd(nhubs, 1)] = j;
}
// Hub lists are sorted by ONE WAVE each when they fit its share of the LDS buffer (wave-level synchronisation only: with one
// workgroup per hub, 28 workgroup barriers went into a 100-entry list), by the whole workgroup otherwise.  Three launches of the
// same kernel: lists of up to 1024 entries with a 16 KB buffer (ten workgroups = 40 lists in flight per CU - nearly all hubs:
// with the 64 KB buffer of the longest lists two workgroups fitted, and a batch with ~10^4 hubs of a few hundred entries
// spent 0.63 ms here), then up to 4096 per wave, then up to 16384 per workgroup.
// One compare-exchange step of a bitonic network on buf[0..P): thread slot i of NT handles pairs i, i + NT, ...
template <int NT>
__device__ __forceinline__ void rev_bitonic_step(int* buf, int P, int k, int jj, int slot) {
    for (int t = slot; t < (P >> 1); t += NT) {
        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));      // the pair's lower index: bit jj clear
        const int p = i | jj;
        const int a = buf[i], b = buf[p];
        if ((a > b) == ((i & k) == 0)) { buf[i] = b; buf[p] = a; }
    }
}
// WAVE_CAP: longest list one wave sorts (LDS = 4 * WAVE_CAP ints); lists in (lo_len, WAVE_CAP] are this launch's;
// WG_CAP > 0: lists in (WAVE_CAP, WG_CAP] are sorted by the whole workgroup in the same buffer (WG_CAP <= 4 * WAVE_CAP)
template <int WAVE_CAP, int WG_CAP>
__global__ __launch_bounds__(256) void rev_sort_kernel(const int* __restrict__ rev_ptr, const int* __restrict__ hubs,
                                                       const int* __restrict__ nhubs, int* __restrict__ rev_rows, int lo_len) {
    __shared__ int buf[4 * WAVE_CAP];
    const int n = *nhubs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        int* wb = buf + wave * WAVE_CAP;
        for (int t = blockIdx.x * 4 + wave; t < n; t += gridDim.x * 4) {
            const int j = hubs[t];
            const int lo = rev_ptr[j], d = rev_ptr[j + 1] - lo;
            if (d <= lo_len || d > WAVE_CAP) continue;               // another launch / the second pass
            int P = 128;
            while (P < d) P <<= 1;
            for (int i = lane; i < P; i += 64) wb[i] = i < d ? rev_rows[lo + i] : 0x7fffffff;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k = 2; k <= P; k <<= 1)
                for (int jj = k >> 1; jj > 0; jj >>= 1) {
                    rev_bitonic_step<64>(wb, P, k, jj, lane);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            for (int i = lane; i < d; i += 64) rev_rows[lo + i] = wb[i];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    if constexpr (WG_CAP > 0) {
        __syncthreads();
        for (int t = blockIdx.x; t < n; t += gridDim.x) {
            const int j = hubs[t];
            const int lo = rev_ptr[j], d = rev_ptr[j + 1] - lo;
            if (d <= WAVE_CAP || d > WG_CAP) continue;               // (workgroup-uniform)
            int P = 128;
            while (P < d) P <<= 1;
            for (int i = threadIdx.x; i < P; i += 256) buf[i] = i < d ? rev_rows[lo + i] : 0x7fffffff;
            __syncthreads();
            for (int k = 2; k <= P; k <<= 1)
                for (int jj = k >> 1; jj > 0; jj >>= 1) {
                    rev_bitonic_step<256>(buf, P, k, jj, (int)threadIdx.x);
                    __syncthreads();
                }
            for (int i = threadIdx.x; i < d; i += 256) rev_rows[lo + i] = buf[i];
            __syncthreads();
        }
    }
}
static void launch_rev_sort(const int* rev_ptr, const int* hubs, const int* nhubs, int* rev_rows, int N, hipStream_t st) {
    const dim3 grid(N < 2560 ? (N < 1 ? 1 : N) : 2560), block(256);
    hipLaunchKernelGGL((rev_sort_kernel<1024, 0>), grid, block, 0, st, rev_ptr, hubs, nhubs, rev_rows, REV_SORT_MIN);
    if (N > 1024) hipLaunchKernelGGL((rev_sort_kernel<REV_SORT_CAP / 4, REV_SORT_CAP>), dim3(N < 512 ? N : 512), block, 0, st, rev_ptr, hubs, nhubs,
                                     rev_rows, 1024);
}

// ---------------------------------------------------------------- edge_index <-> table
__global__ __launch_bounds__(256) void table_degree(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                    int N, int K, int* __restrict__ deg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    int c = 0;
    for (int s = 0; s < K; ++s) c += nbr[(long long)i * K + s] >= 0;
    if (ovf) c += ovf[i] >= 0;
    deg[i] = c;
}
__global__ __launch_bounds__(256) void table_to_edges(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                      int N, int K, const int* __restrict__ off, long long E,
                                                      long long* __restrict__ edge_index) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    long long e = off[i];
    for (int s = 0; s < K; ++s) {
        const int j = nbr[(long long)i * K + s];
        if (j >= 0) { edge_index[e] = j; edge_index[E + e] = i; ++e; }
    }
    if (ovf && ovf[i] >= 0) { edge_index[e] = ovf[i]; edge_index[E + e] = i; }
}
// edges sorted by target (edge_index[1] ascending, as knn_graph emits them): the e-th edge of
// centre i goes to slot e - first[i]; slot K goes to ovf.  Nothing is written from an entry that has not been
// validated: pass 1 range-checks BOTH rows of the int64 input (before any truncation to int) and the order, pass 2
// does not run at all when pass 1 raised a flag.  *err bits: 1 = an index outside [0, N), 2 = not grouped by
// ascending target, 4 = an in-degree above K + 1 (the host side re-sorts / re-sizes and calls again).
__global__ __launch_bounds__(256) void edges_first(const long long* __restrict__ src, const long long* __restrict__ dst,
                                                   long long E, int N, int* __restrict__ first, int* __restrict__ err) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const long long d = dst[e], s = src[e];
    if (d < 0 || d >= N || s < 0 || s >= N) { atomicOr(err, 1); return; }
    if (e > 0 && dst[e - 1] > d) atomicOr(err, 2);
    if (e == 0 || dst[e - 1] != d) first[d] = (int)e;             // one writer per target when the order is right
}
__global__ __launch_bounds__(256) void edges_to_table(const long long* __restrict__ src, const long long* __restrict__ dst,
                                                      long long E, const int* __restrict__ first, int K,
                                                      int* __restrict__ nbr, int* __restrict__ ovf, int* __restrict__ err) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    if ((__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 3) != 0) return;   // pass 1 refused the input
    const int i = (int)dst[e];
    const long long s = e - first[i];                              // >= 0: targets ascend and first[i] is i's run start
    if (s < 0) { atomicOr(err, 2); return; }
    if (s < K) nbr[(long long)i * K + s] = (int)src[e];
    else if (s == K) ovf[i] = (int)src[e];
    else atomicOr(err, 4);                                         // degree > K+1
}

// ---------------------------------------------------------------- feature standardisation
// Detector._standardize (models/detector/detector.py:64-77) for a whole batch in one pass, in place: column f
// runs its program of up to 3 steps (add / sub / mul / div / log10 with a constant), in fp32, in the order
// and with the operations of the reference's per-column lambdas (icecube.py:21-48, prometheus.py:11-39).
constexpr int STD_MAXF = 32, STD_MAXOPS = 3;
struct StdProgram { int nops[STD_MAXF]; int op[STD_MAXF][STD_MAXOPS]; float c[STD_MAXF][STD_MAXOPS]; };
__global__ __launch_bounds__(256) void standardize_kernel(float* __restrict__ x, long long ldx, int N, int F, StdProgram p) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / F), f = (int)(t % F);
    if (i >= N) return;
    float v = x[(long long)i * ldx + f];
    const int n = p.nops[f];
    for (int k = 0; k < STD_MAXOPS; ++k) {
        if (k < n) {
            const float c = p.c[f][k];
            switch (p.op[f][k]) {
                case 0: v = v + c; break;
                case 1: v = v - c; break;
                case 2: v = v * c; break;
                case 3: v = v / c; break;
                default: v = log10f(v); break;
            }
        }
    }
    x[(long long)i * ldx + f] = v;
}

// ---------------------------------------------------------------- global variables
// One workgroup (4 waves) per event.  out[g, 0:F] = mean_i x[i,:], out[g, F+c] = homophily of column c
// (c = 0..3; exact float equality over edges j->i of the event), out[g, F+4] = log10(n).
// An event is summed in SLICES of EVENT_SLICE consecutive pulses (thread t takes pulses lo+t, lo+t+256, ... of the slice;
// lanes are combined by a butterfly, the 4 waves in wave order), the slices are added in order: the result of an event
// depends on that event alone, and an event of up to EVENT_SLICE pulses is one slice.  PART = false: one workgroup walks
// the slices of its event; PART = true (a batch of a few huge events): workgroup (g, blockIdx.y) sums ONE slice into
// `part` ([B * SMAX][GLOB_REC] words) and globals_combine_kernel adds the slices - same operations, same order.
constexpr int EVENT_SLICE = 1024;                          // = pool.hip
constexpr int GLOB_FMAX = 32, GLOB_REC = GLOB_FMAX + 5;
template <bool PART>
__global__ __launch_bounds__(256) void globals_kernel(
    const float* __restrict__ x, long long ldx, int F, const int* __restrict__ ptr, int B, int SMAX,
    const int* __restrict__ nbr, const int* __restrict__ ovf, int K,
    const int* __restrict__ n_pulses, float* __restrict__ out, float* __restrict__ part)
{
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ev_lo = ptr[g], ev_hi = ptr[g + 1];
    const int nsl = max((ev_hi - ev_lo + EVENT_SLICE - 1) / EVENT_SLICE, 1);
    if (PART && (int)blockIdx.y >= nsl) return;
    constexpr int FMAX = GLOB_FMAX;
    __shared__ float s_sum[4][FMAX];
    __shared__ int s_cnt[4][5];
    float rsum[FMAX];                                       // running sums over the slices (thread 0)
    int rcnt[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int f = 0; f < FMAX; ++f) rsum[f] = 0.0f;
    const int sl0 = PART ? (int)blockIdx.y : 0, sl1 = PART ? (int)blockIdx.y + 1 : nsl;
    for (int sl = sl0; sl < sl1; ++sl) {
        const int lo = ev_lo + sl * EVENT_SLICE, hi = min(lo + EVENT_SLICE, ev_hi);
        float sum[FMAX];
#pragma unroll
        for (int f = 0; f < FMAX; ++f) sum[f] = 0.0f;
        int match[4] = {0, 0, 0, 0};
        int edges = 0;
        for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
            const float* xi = x + (long long)i * ldx;
#pragma unroll
            for (int f = 0; f < FMAX; ++f) if (f < F) sum[f] += xi[f];
            const float a0 = xi[0], a1 = xi[1], a2 = xi[2], a3 = xi[3];
            for (int s = 0; s <= K; ++s) {
                int j;
                if (s < K) j = nbr[(long long)i * K + s];
                else j = ovf ? ovf[i] : -1;
                if (j < 0) continue;
                const float* xj = x + (long long)j * ldx;
                ++edges;
                match[0] += (xj[0] == a0);
                match[1] += (xj[1] == a1);
                match[2] += (xj[2] == a2);
                match[3] += (xj[3] == a3);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int f = 0; f < FMAX; ++f) if (f < F) sum[f] += __shfl_xor(sum[f], o);
#pragma unroll
            for (int c = 0; c < 4; ++c) match[c] += __shfl_xor(match[c], o);
            edges += __shfl_xor(edges, o);
        }
        if (sl > sl0) __syncthreads();                     // thread 0 has read the previous slice's records
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < FMAX; ++f) s_sum[wave][f] = sum[f];
#pragma unroll
            for (int c = 0; c < 4; ++c) s_cnt[wave][c] = match[c];
            s_cnt[wave][4] = edges;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int f = 0; f < F; ++f) {
                const float v = ((s_sum[0][f] + s_sum[1][f]) + s_sum[2][f]) + s_sum[3][f];
                rsum[f] = sl == 0 ? v : rsum[f] + v;       // (a one-slice event keeps the bits of the plain sum)
            }
            for (int c = 0; c < 5; ++c) rcnt[c] += s_cnt[0][c] + s_cnt[1][c] + s_cnt[2][c] + s_cnt[3][c];
        }
    }
    if (threadIdx.x != 0) return;
    if constexpr (PART) {
        float* rec = part + ((long long)g * SMAX + blockIdx.y) * GLOB_REC;
        for (int f = 0; f < F; ++f) rec[f] = rsum[f];
        for (int c = 0; c < 5; ++c) reinterpret_cast<int*>(rec)[FMAX + c] = rcnt[c];
        return;
    }
    const int G = F + 5;
    float* o = out + (long long)g * G;
    const float cnt = (float)max(ev_hi - ev_lo, 1);
    for (int f = 0; f < F; ++f) o[f] = rsum[f] / cnt;
    const float ne = (float)max(rcnt[4], 1);
    for (int c = 0; c < 4; ++c) o[F + c] = (float)rcnt[c] / ne;
    o[F + 4] = log10f((float)n_pulses[g]);
}
__global__ __launch_bounds__(64) void globals_combine_kernel(const int* __restrict__ ptr, int F, int SMAX, const int* __restrict__ n_pulses,
                                                             const float* __restrict__ part, float* __restrict__ out) {
    const int g = blockIdx.x, t = threadIdx.x;
    const int n = ptr[g + 1] - ptr[g];
    const int nsl = max((n + EVENT_SLICE - 1) / EVENT_SLICE, 1);
    float* o = out + (long long)g * (F + 5);
    if (t < F) {
        float s = 0.0f;
        for (int sl = 0; sl < nsl; ++sl) {
            const float v = part[((long long)g * SMAX + sl) * GLOB_REC + t];
            s = sl == 0 ? v : s + v;
        }
        o[t] = s / (float)max(n, 1);
    } else if (t < F + 4) {
        int m = 0, ed = 0;
        for (int sl = 0; sl < nsl; ++sl) {
            const int* rec = reinterpret_cast<const int*>(part + ((long long)g * SMAX + sl) * GLOB_REC);
            m += rec[GLOB_FMAX + (t - F)];
            ed += rec[GLOB_FMAX + 4];
        }
        o[t] = (float)m / (float)max(ed, 1);
    } else if (t == F + 4) {
        o[t] = log10f((float)n_pulses[g]);
    }
}

// x0[i, 0:F] = x[i,:], x0[i, F:F+G] = gv[batch[i], :], zero padding up to ld0 columns.
template <typename OutT>
__global__ __launch_bounds__(256) void concat_globals(const float* __restrict__ x, long long ldx, int F,
                                                      const float* __restrict__ gv, int G,
                                                      const int* __restrict__ batch, int N,
                                                      OutT* __restrict__ x0, int ld0) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t / ld0), c = (int)(t % ld0);
    if (i >= N) return;
    float v = 0.0f;
    if (c < F) v = x[(long long)i * ldx + c];
    else if (c < F + G) v = gv[(long long)batch[i] * G + (c - F)];
    x0[(long long)i * ld0 + c] = from_f32<OutT>(v);
}

__global__ __launch_bounds__(256) void ptr_to_batch(const int* __restrict__ ptr, int B, int* __restrict__ batch) {
    const int g = blockIdx.x;
    for (int i = ptr[g] + threadIdx.x; i < ptr[g + 1]; i += 256) batch[i] = g;
}

}  // namespace gn

// =============================================================== host launchers (C++ linkage)
namespace gn {

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

hipError_t launch_knn_plan(const int* ptr, int B, int* tile_ptr, hipStream_t st) {
    hipLaunchKernelGGL(knn_plan_kernel, dim3(1), dim3(256), 0, st, ptr, B, tile_ptr);
    return hipGetLastError();
}

struct KnnSweepWs { int* sidx; float* sx; float* bbox; int* bminj; long long total; };
static KnnSweepWs knn_ws_layout(void* ws, int B, int N, int D) {
    KnnSweepWs L;
    unsigned char* base = static_cast<unsigned char*>(ws);
    auto al = [](long long v) { return (v + 255) / 256 * 256; };
    long long off = 0;
    L.sidx = reinterpret_cast<int*>(base + off); off += al((long long)N * 4);
    L.sx = reinterpret_cast<float*>(base + off); off += al((long long)N * D * 4);
    L.bbox = reinterpret_cast<float*>(base + off); off += al(((long long)N / KNN_TILE + B) * KNN_BOX * 4);
    L.bminj = reinterpret_cast<int*>(base + off); off += al(((long long)N / KNN_TILE + B) * 4);
    L.total = off;
    return L;
}
long long knn_ws_bytes(int B, int N, int D) { return knn_ws_layout(nullptr, B, N, D < 1 ? 1 : D).total; }
static int knn_sweep_min() {            // GN_KNN_SWEEP_MIN=<pulses>: events above it take the sorted sweep; 0 = never
    static const int v = [] { const char* e = getenv("GN_KNN_SWEEP_MIN"); const int u = e ? atoi(e) : KNN_SWEEP_MIN; return u <= 0 ? KNN_SWEEP_MAX : u; }();
    return v;
}

// ws: knn_ws_bytes(B, N, D) of scratch, or nullptr (every event scanned exhaustively)
hipError_t launch_knn(const float* x, long long ldx, const int* cols, int D, const int* ptr, const int* tile_ptr,
                      int B, int N, int k, int strict, int* nbr, int* ovf, void* ws, hipStream_t st) {
    if (N == 0 || B == 0) return hipSuccess;
    KnnCols kc;
    for (int d = 0; d < KNN_DMAX; ++d) kc.c[d] = d < D ? cols[d] : 0;
    const int kk = k + 1;                                   // list length in both modes (strict drops the query at the end)
    // upper bound of sum ceil(n_e/64) known without reading ptr on the host; surplus workgroups exit at once
    const long long tiles = (long long)N / KNN_TILE + B;
    dim3 grid((unsigned)tiles), block(KNN_TILE);
    // the sweep's two launches only where large events are the rule (the host does not know the event sizes)
    const bool sweep = ws && (long long)N >= (long long)KNN_SWEEP_AVG * B && N > knn_sweep_min() && knn_sweep_min() < KNN_SWEEP_MAX;
    const int smin = sweep ? knn_sweep_min() : KNN_SWEEP_MAX;            // n > KNN_SWEEP_MAX is never owned by the sweep
    KnnSweepWs L = knn_ws_layout(ws, B, N, D);
    if (sweep) {
        if (D == 3) hipLaunchKernelGGL((knn_sort_kernel<3>), dim3(B), dim3(1024), 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, smin, L.sidx, L.sx, L.bbox, L.bminj);
        else hipLaunchKernelGGL((knn_sort_kernel<0>), dim3(B), dim3(1024), 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, smin, L.sidx, L.sx, L.bbox, L.bminj);
    }
#define GN_KNN_LAUNCH(KM)                                                                                       \
    {                                                                                                           \
        const dim3 blockb(KNN_TILE * 8), gridb(1024);        /* second launch: events above KNN_BIG pulses */   \
        if (D == 3) {                                                                                           \
            hipLaunchKernelGGL((knn_kernel<KM, 3, 1>), grid, block, 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, k, \
                               strict, smin, nbr, ovf, KnnMetric<0>());                                        \
            if (bigpossible)                                                                                    \
                hipLaunchKernelGGL((knn_kernel<KM, 3, 8>), gridb, blockb, 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, \
                                   k, strict, smin, nbr, ovf, KnnMetric<0>());                                 \
            if (sweep)                                                                                          \
                hipLaunchKernelGGL((knn_sweep_kernel<KM, 3>), grid, block, 0, st, D, ptr, tile_ptr, B, N, k, strict, \
                                   smin, L.sidx, L.sx, L.bbox, L.bminj, nbr, ovf);                              \
        } else {                                                                                                \
            hipLaunchKernelGGL((knn_kernel<KM, 0, 1>), grid, block, 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, k, \
                               strict, smin, nbr, ovf, KnnMetric<0>());                                        \
            if (bigpossible)                                                                                    \
                hipLaunchKernelGGL((knn_kernel<KM, 0, 8>), gridb, blockb, 0, st, x, ldx, kc, D, ptr, tile_ptr, B, N, \
                                   k, strict, smin, nbr, ovf, KnnMetric<0>());                                 \
            if (sweep)                                                                                          \
                hipLaunchKernelGGL((knn_sweep_kernel<KM, 0>), grid, block, 0, st, D, ptr, tile_ptr, B, N, k, strict, \
                                   smin, L.sidx, L.sx, L.bbox, L.bminj, nbr, ovf);                              \
        }                                                                                                       \
    }
    const bool bigpossible = N > KNN_BIG;                   // an event can only be that large if the batch is
    if (kk <= 9) GN_KNN_LAUNCH(9)
    else if (kk <= 17) GN_KNN_LAUNCH(17)
    else GN_KNN_LAUNCH(33)
#undef GN_KNN_LAUNCH
    return hipGetLastError();
}

// k-NN under the Minkowski metric (KnnMetric<1>): the strict table nbr[N, k], degree min(k, n - 1), ascending (m, j).
// Always the exhaustive scan, whatever the event sizes (see knn_tile): one launch, plus the 8-wave launch when the batch
// can hold an event above KNN_BIG pulses.  Lists of 8 / 16 / 32 entries: k of them are written.
hipError_t launch_minkowski_knn(const float* x, long long ldx, const int* space_cols, int DS, int time_col, float c,
                                float time_like_weight, const int* ptr, const int* tile_ptr, int B, int N, int k, int* nbr,
                                hipStream_t st) {
    if (N == 0 || B == 0) return hipSuccess;
    KnnCols kc;
    for (int d = 0; d < KNN_DMAX; ++d) kc.c[d] = d < DS ? space_cols[d] : 0;
    KnnMetric<1> mk;
    mk.tcol = time_col; mk.c = c; mk.ntlw = -time_like_weight;
    const long long tiles = (long long)N / KNN_TILE + B;
    const dim3 grid((unsigned)tiles), block(KNN_TILE), blockb(KNN_TILE * 8), gridb(1024);
    const bool bigpossible = N > KNN_BIG;
    int* const no_ovf = nullptr;
#define GN_MINK_LAUNCH(KM, DT_)                                                                                 \
    {                                                                                                           \
        hipLaunchKernelGGL((knn_kernel<KM, DT_, 1, 1>), grid, block, 0, st, x, ldx, kc, DS, ptr, tile_ptr, B, N, k, 1, \
                           KNN_SWEEP_MAX, nbr, no_ovf, mk);                                                     \
        if (bigpossible)                                                                                        \
            hipLaunchKernelGGL((knn_kernel<KM, DT_, 8, 1>), gridb, blockb, 0, st, x, ldx, kc, DS, ptr, tile_ptr, B, N, \
                               k, 1, KNN_SWEEP_MAX, nbr, no_ovf, mk);                                           \
    }
#define GN_MINK_LAUNCH_K(DT_)                                                                                   \
    {                                                                                                           \
        if (k <= 8) GN_MINK_LAUNCH(8, DT_)                                                                      \
        else if (k <= 16) GN_MINK_LAUNCH(16, DT_)                                                               \
        else GN_MINK_LAUNCH(32, DT_)                                                                            \
    }
    if (DS == 3) GN_MINK_LAUNCH_K(3)
    else GN_MINK_LAUNCH_K(0)
#undef GN_MINK_LAUNCH_K
#undef GN_MINK_LAUNCH
    return hipGetLastError();
}

// Radius graph: nbr[N, cap] and deg[N] (see radius_append_kernel).  Two launches on the tile plan, always: the second one
// finds its work list empty when no centre is above the cap.  work: radius_work_ints(B, N) ints.
long long radius_work_ints(int B, int N) { return 1 + (long long)N / KNN_TILE + B; }
hipError_t launch_radius_graph(const float* x, long long ldx, const int* cols, int D, float r, const int* ptr,
                               const int* tile_ptr, int B, int N, int cap, int* nbr, int* deg, int* work, hipStream_t st) {
    if (N == 0 || B == 0) return hipSuccess;
    KnnCols kc;
    for (int d = 0; d < KNN_DMAX; ++d) kc.c[d] = d < D ? cols[d] : 0;
    const float r2 = r * r;
    hipError_t e = hipMemsetAsync(work, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    const long long tiles = (long long)N / KNN_TILE + B;
    const dim3 grid((unsigned)tiles), block(KNN_TILE), grido((unsigned)(tiles < 2048 ? tiles : 2048));
#define GN_RADIUS_LAUNCH(KM, DT_)                                                                               \
    hipLaunchKernelGGL((radius_overflow_kernel<KM, DT_>), grido, block, 0, st, x, ldx, kc, D, r2, ptr, tile_ptr, B, N, cap, \
                       nbr, deg, work);
#define GN_RADIUS_LAUNCH_D(DT_)                                                                                 \
    {                                                                                                           \
        hipLaunchKernelGGL((radius_append_kernel<DT_>), grid, block, 0, st, x, ldx, kc, D, r2, ptr, tile_ptr, B, N, cap, \
                           nbr, deg, work);                                                                     \
        if (cap <= 8) GN_RADIUS_LAUNCH(8, DT_)                                                                  \
        else if (cap <= 16) GN_RADIUS_LAUNCH(16, DT_)                                                           \
        else GN_RADIUS_LAUNCH(32, DT_)                                                                          \
    }
    if (D == 3) GN_RADIUS_LAUNCH_D(3)
    else GN_RADIUS_LAUNCH_D(0)
#undef GN_RADIUS_LAUNCH_D
#undef GN_RADIUS_LAUNCH
    return hipGetLastError();
}

// out[i] = sum_{t<i} in[i]; total (optional) = sum of all.  tmp: >= cdiv(n, 2048) ints.
// exclusive scan of in[] (flag = false) or of the predicate in[i] >= 0 (flag = true)
static hipError_t launch_scan_impl(const int* in, int* out, int n, int* tmp, int* total, bool flag, hipStream_t st) {
    const int per = SCAN_BLOCK * SCAN_ITEMS;
    const int nb = cdiv(n > 0 ? n : 1, per);
    int* total1 = nb == 1 ? total : nullptr;
    if (flag) hipLaunchKernelGGL(scan_phase1<true>, dim3(nb), dim3(SCAN_BLOCK), 0, st, in, n, out, tmp, total1);
    else hipLaunchKernelGGL(scan_phase1<false>, dim3(nb), dim3(SCAN_BLOCK), 0, st, in, n, out, tmp, total1);
    if (nb == 1) return hipGetLastError();             // one block: done (the per-event edge counts of batches up to 2048 slices)
    if (nb <= 1024) {                                  // two launches: each block adds up the block totals before it
        hipLaunchKernelGGL(scan_phase23, dim3(nb), dim3(SCAN_BLOCK), 0, st, out, n, tmp, total);
    } else {
        hipLaunchKernelGGL(scan_phase2, dim3(1), dim3(SCAN_BLOCK), 0, st, tmp, nb, total);
        hipLaunchKernelGGL(scan_phase3, dim3(nb), dim3(SCAN_BLOCK), 0, st, out, n, tmp);
    }
    return hipGetLastError();
}
hipError_t launch_scan(const int* in, int* out, int n, int* tmp, int* total, hipStream_t st) {
    return launch_scan_impl(in, out, n, tmp, total, false, st);
}

hipError_t launch_ovf_compact(const int* ovf, int N, int* flag_pos /*[N]*/, int* tmp, int* ovf_centre, int* ovf_src,
                              int* ovf_cnt, hipStream_t st) {
    if (N == 0) return hipMemsetAsync(ovf_cnt, 0, sizeof(int), st);
    hipError_t e = launch_scan_impl(ovf, flag_pos, N, tmp, ovf_cnt, true, st);      // positions of the entries >= 0
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ovf_write, dim3(cdiv(N, 256)), dim3(256), 0, st, ovf, flag_pos, N, ovf_centre, ovf_src);
    return hipGetLastError();
}

// ---- event-local build: graphs whose edges never leave an event (everything gn_knn_graph produces) ----
// One workgroup per event does count, scan and fill with the in-degree counters in LDS (events of up to
// REV_EV_CAP pulses; larger ones use the event's slice of a global scratch array, same code): 3 launches that read
// the neighbour table twice instead of the global path's count / scan / fill / hub search over N atomics in HBM.
// ovf[i] = source of centre i's (k+1)-th edge or -1; ovf_pos[i] = index of that overflow row (row id N*S + ovf_pos[i]).
constexpr int REV_EV_CAP = 8192;
// Scan of the table entries [a, b) of an event by the 256 threads of a workgroup: the loads of 4 x 4 entries are issued
// before any is looked at (the body has a data-dependent branch; one load per iteration left every wave waiting a
// full L2 round trip per entry: 0.53 ms for the 1.7e5 entries of a 10^4-pulse event).
#define GN_SCAN_TABLE(nbr_, a_, b_, tid_, NT_, ...)                                                        \
    {                                                                                                 \
        const long long a__ = (a_), b__ = (b_);                                                       \
        const long long a4__ = (a__ + 3) & ~3ll;                     /* first 16-byte aligned entry */ \
        for (long long t = a__ + (tid_); t < (a4__ < b__ ? a4__ : b__); t += (NT_)) { const int j = (nbr_)[t]; __VA_ARGS__ }          \
        for (long long t0 = a4__ + 4ll * (tid_); t0 < b__; t0 += 4ll * (NT_) * 4) {                     \
            int4 v__[4];                                                                              \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                           \
                const long long tu = t0 + 4ll * (NT_) * u;                                              \
                v__[u] = make_int4(-1, -1, -1, -1);                                                   \
                if (tu + 3 < b__) v__[u] = *reinterpret_cast<const int4*>((nbr_) + tu);               \
                else if (tu < b__) { v__[u].x = (nbr_)[tu]; if (tu + 1 < b__) v__[u].y = (nbr_)[tu + 1]; if (tu + 2 < b__) v__[u].z = (nbr_)[tu + 2]; } \
            }                                                                                         \
            _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                           \
                const long long tu = t0 + 4ll * (NT_) * u;                                              \
                { const long long t = tu; const int j = v__[u].x; if (t < b__) { __VA_ARGS__ } }             \
                { const long long t = tu + 1; const int j = v__[u].y; if (t < b__) { __VA_ARGS__ } }         \
                { const long long t = tu + 2; const int j = v__[u].z; if (t < b__) { __VA_ARGS__ } }         \
                { const long long t = tu + 3; const int j = v__[u].w; if (t < b__) { __VA_ARGS__ } }         \
            }                                                                                         \
        }                                                                                             \
    }

// NSL > 1: the sources of an event are cut into NSL contiguous slices and workgroup (e, sl) = blockIdx.x = e * NSL + sl
// builds the lists of slice sl only, scanning ALL rows of its event (redundant reads of the small neighbour table, no
// communication between the slices).  A batch of a few huge events (BASELINE configs[4]: 16 x 10^4 pulses) then
// still fills the chip; with one workgroup per event it ran on 16 CUs, and the global path (N*S contended atomics on
// hub pulses) took 0.93 ms per graph.
// NT threads per workgroup: 256 for ordinary batches (an event per workgroup); 1024 when the events are cut into slices (a
// few huge events): a workgroup then scans ~10^5 table entries and 256 threads left each with 600 dependent iterations
template <int NT>
__global__ __launch_bounds__(NT) void rev_event_count(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                      const int* __restrict__ ptr, int K, int NSL, int* __restrict__ ev_edges,
                                                      int* __restrict__ nhubs) {
    __shared__ int red[NT / 64];
    const int e = (int)blockIdx.x / NSL, sl = (int)blockIdx.x % NSL, lo = ptr[e], hi = ptr[e + 1];
    const int per = (max(hi - lo, 0) + NSL - 1) / NSL;
    const int j0 = lo + sl * per, j1 = min(j0 + per, hi);          // sources of this slice
    int c = 0;
    // (NSL == 1: [j0, j1) is the whole event and every entry >= 0 lies in it - edges never leave an event)
    GN_SCAN_TABLE(nbr, (long long)lo * K, (long long)hi * K, threadIdx.x, NT, { (void)t; c += (j >= j0 && j < j1) ? 1 : 0; });
    if (ovf) GN_SCAN_TABLE(ovf, (long long)lo, (long long)hi, threadIdx.x, NT, { (void)t; c += (j >= j0 && j < j1) ? 1 : 0; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) tot += red[w];
        ev_edges[blockIdx.x] = tot;
        if (blockIdx.x == 0) *nhubs = 0;
    }
}
template <int NT>
__global__ __launch_bounds__(NT) void rev_event_build(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                      const int* __restrict__ ovf_pos, const int* __restrict__ ptr,
                                                      const int* __restrict__ ev_base, int B, int N, int K, int S, int NSL,
                                                      int* __restrict__ rev_ptr, int* __restrict__ rev_rows,
                                                      int* __restrict__ scratch, int* __restrict__ hubs,
                                                      int* __restrict__ nhubs) {
    __shared__ int lds_cnt[REV_EV_CAP];
    __shared__ int chunk_sum[256];
    const int e = (int)blockIdx.x / NSL, sl = (int)blockIdx.x % NSL, lo = ptr[e], hi = ptr[e + 1], tid = threadIdx.x;
    const int base = ev_base[blockIdx.x];
    if ((int)blockIdx.x == B * NSL - 1 && tid == 0) rev_ptr[N] = ev_base[B * NSL];
    const int per = (max(hi - lo, 0) + NSL - 1) / NSL;
    const int j0 = lo + sl * per, j1 = min(j0 + per, hi);          // sources of this slice: [j0, j1)
    const int n = j1 - j0;
    if (n <= 0) return;
    int* cnt = n <= REV_EV_CAP ? lds_cnt : scratch + j0;       // workgroup-uniform
    for (int j = tid; j < n; j += NT) cnt[j] = 0;
    __syncthreads();
    GN_SCAN_TABLE(nbr, (long long)lo * K, (long long)hi * K, tid, NT, { (void)t; if (j >= j0 && j < j1) atomicAdd(&cnt[j - j0], 1); });
    if (ovf) GN_SCAN_TABLE(ovf, (long long)lo, (long long)hi, tid, NT, { (void)t; if (j >= j0 && j < j1) atomicAdd(&cnt[j - j0], 1); });
    __threadfence_block();
    __syncthreads();
    // exclusive scan of cnt[0..n): thread t < 256 owns the contiguous piece [t*pp, (t+1)*pp)
    const int pp = (n + 255) / 256;
    const int p0 = min(min(tid, 256) * pp, n), p1 = tid < 256 ? min(p0 + pp, n) : p0;
    int sum = 0;
    for (int j = p0; j < p1; ++j) sum += cnt[j];
    if (tid < 256) chunk_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int t = 0; t < 256; ++t) { const int v = chunk_sum[t]; chunk_sum[t] = run; run += v; } }
    __syncthreads();
    int run = tid < 256 ? chunk_sum[tid] : 0;
    for (int j = p0; j < p1; ++j) {
        const int d = cnt[j];
        cnt[j] = run;                                            // becomes the fill cursor of source j
        rev_ptr[j0 + j] = base + run;
        if (d > REV_SORT_MIN && d <= REV_SORT_CAP) hubs[atomicAdd(nhubs, 1)] = j0 + j;
        run += d;
    }
    __threadfence_block();
    __syncthreads();
    GN_SCAN_TABLE(nbr, (long long)lo * K, (long long)hi * K, tid, NT, {
        if (j >= j0 && j < j1) {
            const int i = (int)(t / K), sk = (int)(t % K);
            rev_rows[base + atomicAdd(&cnt[j - j0], 1)] = i * S + sk;
        }
    });
    if (ovf) GN_SCAN_TABLE(ovf, (long long)lo, (long long)hi, tid, NT, {
        if (j >= j0 && j < j1) rev_rows[base + atomicAdd(&cnt[j - j0], 1)] = N * S + ovf_pos[t];
    });
}

// Huge events (BASELINE configs[4]: 16 x 10^4 pulses, 64 slices per event): the kernels above make every slice workgroup
// read its event's WHOLE table three times - 64-fold redundant, 0.30 ms per graph.  Bucketed build, every entry read twice:
//   rev_bucket_count   workgroup (e, p) scans the p-th part of the event's ROWS and adds, per source slice, the number of
//                      entries it holds to ev_edges[e * NSL + slice]                      (-> scan -> ev_base, as before)
//   rev_bucket_scatter the same scan again: reserves a range per slice in the slice's bucket (one global atomic per
//                      (workgroup, slice)) and writes (source, row id) pairs there - bucket g is pairs[ev_base[g] ..)
//   rev_bucket_build   workgroup (e, sl) = the old rev_event_build on its own bucket only
// The order inside a list is the order the atomics came in, as in rev_event_build (the gather sorts / rev_sort_kernel).
constexpr int REV_BK_NT = 1024;
template <typename F>
__device__ __forceinline__ void rev_bucket_scan(const int* __restrict__ nbr, const int* __restrict__ ovf, const int* __restrict__ ovf_pos,
                                                int r0, int r1, int K, int S, int N, int tid, F&& f) {
    const long long a = (long long)r0 * K, b = (long long)r1 * K;
    for (long long t = a + tid; t < b; t += REV_BK_NT) {
        const int j = nbr[t];
        if (j >= 0) f(j, (int)(t / K) * S + (int)(t % K));
    }
    if (ovf)
        for (int i = r0 + tid; i < r1; i += REV_BK_NT) {
            const int j = ovf[i];
            if (j >= 0) f(j, ovf_pos ? N * S + ovf_pos[i] : 0);
        }
}
__global__ __launch_bounds__(REV_BK_NT) void rev_bucket_count(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                              const int* __restrict__ ptr, int K, int NSL, int* __restrict__ ev_edges,
                                                              int* __restrict__ nhubs) {
    __shared__ int cnt[64];
    const int e = (int)blockIdx.x / NSL, p = (int)blockIdx.x % NSL, lo = ptr[e], hi = ptr[e + 1], tid = threadIdx.x;
    const int per = (max(hi - lo, 0) + NSL - 1) / NSL;
    const int r0 = min(lo + p * per, hi), r1 = min(r0 + per, hi);
    if (tid < 64) cnt[tid] = 0;
    if (blockIdx.x == 0 && tid == 0) *nhubs = 0;
    __syncthreads();
    rev_bucket_scan(nbr, ovf, nullptr, r0, r1, K, 0, 0, tid, [&](int j, int) { atomicAdd(&cnt[(j - lo) / per], 1); });
    __syncthreads();
    if (tid < NSL && cnt[tid] > 0) atomicAdd(&ev_edges[e * NSL + tid], cnt[tid]);
}
__global__ __launch_bounds__(REV_BK_NT) void rev_bucket_scatter(const int* __restrict__ nbr, const int* __restrict__ ovf,
                                                                const int* __restrict__ ovf_pos, const int* __restrict__ ptr,
                                                                const int* __restrict__ ev_base, int N, int K, int S, int NSL,
                                                                int* __restrict__ cursor, int* __restrict__ pj, int* __restrict__ prow) {
    __shared__ int cnt[64];
    __shared__ int off[64];
    const int e = (int)blockIdx.x / NSL, p = (int)blockIdx.x % NSL, lo = ptr[e], hi = ptr[e + 1], tid = threadIdx.x;
    const int per = (max(hi - lo, 0) + NSL - 1) / NSL;
    const int r0 = min(lo + p * per, hi), r1 = min(r0 + per, hi);
    if (tid < 64) cnt[tid] = 0;
    __syncthreads();
    rev_bucket_scan(nbr, ovf, nullptr, r0, r1, K, 0, 0, tid, [&](int j, int) { atomicAdd(&cnt[(j - lo) / per], 1); });
    __syncthreads();
    if (tid < NSL) {
        const int c = cnt[tid];
        off[tid] = ev_base[e * NSL + tid] + (c > 0 ? atomicAdd(&cursor[e * NSL + tid], c) : 0);
        cnt[tid] = 0;
    }
    __syncthreads();
    rev_bucket_scan(nbr, ovf, ovf_pos, r0, r1, K, S, N, tid, [&](int j, int row) {
        const int sl = (j - lo) / per;
        const int at = off[sl] + atomicAdd(&cnt[sl], 1);
        pj[at] = j;
        prow[at] = row;
    });
}
__global__ __launch_bounds__(REV_BK_NT) void rev_bucket_build(const int* __restrict__ pj, const int* __restrict__ prow,
                                                              const int* __restrict__ ptr, const int* __restrict__ ev_base, int B, int N,
                                                              int NSL, int* __restrict__ rev_ptr, int* __restrict__ rev_rows,
                                                              int* __restrict__ scratch, int* __restrict__ hubs, int* __restrict__ nhubs) {
    __shared__ int lds_cnt[REV_EV_CAP];
    __shared__ int chunk_sum[256];
    const int e = (int)blockIdx.x / NSL, sl = (int)blockIdx.x % NSL, lo = ptr[e], hi = ptr[e + 1], tid = threadIdx.x;
    const int base = ev_base[blockIdx.x], end = ev_base[blockIdx.x + 1];
    if ((int)blockIdx.x == B * NSL - 1 && tid == 0) rev_ptr[N] = ev_base[B * NSL];
    const int per = (max(hi - lo, 0) + NSL - 1) / NSL;
    const int j0 = lo + sl * per, j1 = min(j0 + per, hi);          // sources of this slice: [j0, j1)
    const int n = j1 - j0;
    if (n <= 0) return;
    int* cnt = n <= REV_EV_CAP ? lds_cnt : scratch + j0;       // workgroup-uniform
    for (int j = tid; j < n; j += REV_BK_NT) cnt[j] = 0;
    __syncthreads();
    for (int t = base + tid; t < end; t += REV_BK_NT) atomicAdd(&cnt[pj[t] - j0], 1);
    __threadfence_block();
    __syncthreads();
    // exclusive scan of cnt[0..n): thread t < 256 owns the contiguous piece [t*pp, (t+1)*pp)
    const int pp = (n + 255) / 256;
    const int p0 = min(min(tid, 256) * pp, n), p1 = tid < 256 ? min(p0 + pp, n) : p0;
    int sum = 0;
    for (int j = p0; j < p1; ++j) sum += cnt[j];
    if (tid < 256) chunk_sum[tid] = sum;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int t = 0; t < 256; ++t) { const int v = chunk_sum[t]; chunk_sum[t] = run; run += v; } }
    __syncthreads();
    int run = tid < 256 ? chunk_sum[tid] : 0;
    for (int j = p0; j < p1; ++j) {
        const int d = cnt[j];
        cnt[j] = run;                                            // becomes the fill cursor of source j
        rev_ptr[j0 + j] = base + run;
        if (d > REV_SORT_MIN && d <= REV_SORT_CAP) hubs[atomicAdd(nhubs, 1)] = j0 + j;
        run += d;
    }
    __threadfence_block();
    __syncthreads();
    for (int t = base + tid; t < end; t += REV_BK_NT) rev_rows[base + atomicAdd(&cnt[pj[t] - j0], 1)] = prow[t];
}

// Slices per event: enough workgroups to fill the chip, at most 64 (redundant table reads grow with it)
int rev_event_slices(int B) {
    int nsl = (1024 + (B > 0 ? B : 1) - 1) / (B > 0 ? B : 1);
    return nsl < 1 ? 1 : (nsl > 64 ? 64 : nsl);
}
// ev: >= 2*(B*NSL+1) ints of workspace (edges per (event, slice), their exclusive scan), NSL = rev_event_slices(B);
// scratch: [N] ints (slices above REV_EV_CAP sources); hubs: [N] ints, nhubs: [1] (the hub list for
// gn_edgeconv_dq_gather); tmp: scan workspace for B*NSL entries
// pairs: rev_pairs_ints(B, N, K) ints of scratch for the bucketed build of huge events, or nullptr
long long rev_pairs_ints(int B, int N, int K) {
    const int NSL = rev_event_slices(B);
    if (!(NSL > 1 && (long long)N >= 2048LL * B)) return 0;
    return 2 * ((long long)N * K + N) + (long long)B * NSL;
}
hipError_t launch_rev_build_events(const int* nbr, int N, int K, int S, const int* ovf, const int* ovf_pos, const int* ptr,
                                   int B, int* rev_ptr, int* rev_rows, int* ev, int* scratch, int* hubs, int* nhubs,
                                   int* tmp, int* pairs, hipStream_t st) {
    if (N == 0 || B == 0) return hipSuccess;
    if ((long long)N * S + N >= (1ll << 31)) return hipErrorInvalidValue;
    const int NSL = rev_event_slices(B);
    const int G = B * NSL;
    int* ev_edges = ev;
    int* ev_base = ev + (G + 1);
    if (pairs && rev_pairs_ints(B, N, K) > 0) {
        const long long E = (long long)N * K + N;
        int* pj = pairs;
        int* prow = pairs + E;
        int* cursor = pairs + 2 * E;
        hipError_t e0 = hipMemsetAsync(ev_edges, 0, sizeof(int) * (size_t)G, st);
        if (e0 != hipSuccess) return e0;
        e0 = hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)G, st);
        if (e0 != hipSuccess) return e0;
        hipLaunchKernelGGL(rev_bucket_count, dim3(G), dim3(REV_BK_NT), 0, st, nbr, ovf, ptr, K, NSL, ev_edges, nhubs);
        hipError_t e = launch_scan(ev_edges, ev_base, G, tmp, ev_base + G, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(rev_bucket_scatter, dim3(G), dim3(REV_BK_NT), 0, st, nbr, ovf, ovf_pos, ptr, ev_base, N, K, S, NSL, cursor, pj, prow);
        hipLaunchKernelGGL(rev_bucket_build, dim3(G), dim3(REV_BK_NT), 0, st, pj, prow, ptr, ev_base, B, N, NSL, rev_ptr, rev_rows, scratch,
                           hubs, nhubs);
        launch_rev_sort(rev_ptr, hubs, nhubs, rev_rows, N, st);
        return hipGetLastError();
    }
    // sliced AND huge events (configs[4]: 16 x 10^4 pulses): 1024 threads scan an event's table; a small batch of ordinary
    // events is sliced too (B = 256: 4 slices of ~40 pulses) and is served better by 256 (29 -> 15 us per graph)
    const bool wide = NSL > 1 && (long long)N >= 2048LL * B;
    if (wide) hipLaunchKernelGGL(rev_event_count<1024>, dim3(G), dim3(1024), 0, st, nbr, ovf, ptr, K, NSL, ev_edges, nhubs);
    else hipLaunchKernelGGL(rev_event_count<256>, dim3(G), dim3(256), 0, st, nbr, ovf, ptr, K, NSL, ev_edges, nhubs);
    hipError_t e = launch_scan(ev_edges, ev_base, G, tmp, ev_base + G, st);
    if (e != hipSuccess) return e;
    if (wide) hipLaunchKernelGGL(rev_event_build<1024>, dim3(G), dim3(1024), 0, st, nbr, ovf, ovf_pos, ptr, ev_base, B, N, K, S, NSL, rev_ptr,
                                 rev_rows, scratch, hubs, nhubs);
    else hipLaunchKernelGGL(rev_event_build<256>, dim3(G), dim3(256), 0, st, nbr, ovf, ovf_pos, ptr, ev_base, B, N, K, S, NSL, rev_ptr,
                            rev_rows, scratch, hubs, nhubs);
    launch_rev_sort(rev_ptr, hubs, nhubs, rev_rows, N, st);
    return hipGetLastError();
}

hipError_t launch_rev_build(const int* nbr, int N, int K, int S, const int* ovf_src, const int* ovf_cnt,
                            int* rev_ptr /*[N+1]*/, int* cursor /*[N]*/, int* tmp, int* rev_rows, hipStream_t st) {
    if (N == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(cursor, 0, sizeof(int) * (size_t)N, st);
    if (e != hipSuccess) return e;
    const long long rows = (long long)N * S + (ovf_cnt ? N : 0);
    hipLaunchKernelGGL(rev_count, dim3(cdiv(rows, 256)), dim3(256), 0, st, nbr, N, K, S, ovf_src, ovf_cnt, cursor);
    e = launch_scan(cursor, rev_ptr, N, tmp, rev_ptr + N, st);
    if (e != hipSuccess) return e;
    // cursor still holds the in-degrees (the scan is out of place): rev_fill counts them down to zero
    hipLaunchKernelGGL(rev_fill, dim3(cdiv(rows, 256)), dim3(256), 0, st, nbr, N, K, S, ovf_src, ovf_cnt, rev_ptr, cursor,
                       rev_rows, tmp);
    // hub nodes (in-degree > 64): sort their lists once; `cursor` (all zero now) receives the hub list, tmp[0] its length
    hipLaunchKernelGGL(rev_find_hubs, dim3(cdiv(N, 256)), dim3(256), 0, st, rev_ptr, N, cursor, tmp);
    launch_rev_sort(rev_ptr, cursor, tmp, rev_rows, N, st);
    return hipGetLastError();
}

hipError_t launch_table_degree(const int* nbr, const int* ovf, int N, int K, int* deg, hipStream_t st) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(table_degree, dim3(cdiv(N, 256)), dim3(256), 0, st, nbr, ovf, N, K, deg);
    return hipGetLastError();
}
hipError_t launch_table_to_edges(const int* nbr, const int* ovf, int N, int K, const int* off, long long E,
                                 long long* edge_index, hipStream_t st) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(table_to_edges, dim3(cdiv(N, 256)), dim3(256), 0, st, nbr, ovf, N, K, off, E, edge_index);
    return hipGetLastError();
}
hipError_t launch_edges_to_table(const long long* edge_index, long long E, int N, int K, int* first /*[N]*/,
                                 int* nbr, int* ovf, int* err, hipStream_t st) {
    hipError_t e = hipMemsetAsync(nbr, 0xff, sizeof(int) * (size_t)N * K, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(ovf, 0xff, sizeof(int) * (size_t)N, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(err, 0, sizeof(int), st);
    if (e != hipSuccess || E == 0) return e;
    hipLaunchKernelGGL(edges_first, dim3(cdiv(E, 256)), dim3(256), 0, st, edge_index, edge_index + E, E, N, first, err);
    hipLaunchKernelGGL(edges_to_table, dim3(cdiv(E, 256)), dim3(256), 0, st, edge_index, edge_index + E, E, first, K, nbr, ovf, err);
    return hipGetLastError();
}

int event_slices_max(int B, int N);                 // pool.hip
long long globals_scratch_bytes(int B, int N) { return (long long)B * event_slices_max(B, N) * GLOB_REC * 4; }
hipError_t launch_globals(const float* x, long long ldx, int F, const int* ptr, int B, const int* nbr, const int* ovf,
                          int K, const int* n_pulses, float* out, hipStream_t st, void* scratch, int N) {
    if (B == 0) return hipSuccess;
    const int SMAX = event_slices_max(B, N);
    if (scratch && SMAX > 1 && F + 5 <= 64) {
        hipLaunchKernelGGL(globals_kernel<true>, dim3(B, SMAX), dim3(256), 0, st, x, ldx, F, ptr, B, SMAX, nbr, ovf, K, n_pulses, out,
                           (float*)scratch);
        hipLaunchKernelGGL(globals_combine_kernel, dim3(B), dim3(64), 0, st, ptr, F, SMAX, n_pulses, (const float*)scratch, out);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(globals_kernel<false>, dim3(B), dim3(256), 0, st, x, ldx, F, ptr, B, 1, nbr, ovf, K, n_pulses, out, (float*)nullptr);
    return hipGetLastError();
}
hipError_t launch_concat_globals(const float* x, long long ldx, int F, const float* gv, int G, const int* batch, int N,
                                 void* x0, int ld0, int out_lowp, hipStream_t st) {
    if (N == 0) return hipSuccess;
    const dim3 grid(cdiv((long long)N * ld0, 256)), block(256);
    if (out_lowp)
        hipLaunchKernelGGL(concat_globals<__bf16>, grid, block, 0, st, x, ldx, F, gv, G, batch, N, (__bf16*)x0, ld0);
    else
        hipLaunchKernelGGL(concat_globals<float>, grid, block, 0, st, x, ldx, F, gv, G, batch, N, (float*)x0, ld0);
    return hipGetLastError();
}
hipError_t launch_standardize(float* x, long long ldx, int N, int F, const int* nops, const int* op, const float* c,
                              hipStream_t st) {
    if (F < 1 || F > STD_MAXF) return hipErrorInvalidValue;
    if (N == 0) return hipSuccess;
    StdProgram p;
    for (int f = 0; f < STD_MAXF; ++f) {
        p.nops[f] = f < F ? nops[f] : 0;
        if (p.nops[f] < 0 || p.nops[f] > STD_MAXOPS) return hipErrorInvalidValue;
        for (int k = 0; k < STD_MAXOPS; ++k) {
            p.op[f][k] = (f < F && k < p.nops[f]) ? op[f * STD_MAXOPS + k] : 0;
            p.c[f][k] = (f < F && k < p.nops[f]) ? c[f * STD_MAXOPS + k] : 0.0f;
            if (p.op[f][k] < 0 || p.op[f][k] > 4) return hipErrorInvalidValue;
        }
    }
    hipLaunchKernelGGL(standardize_kernel, dim3(cdiv((long long)N * F, 256)), dim3(256), 0, st, x, ldx, N, F, p);
    return hipGetLastError();
}
hipError_t launch_ptr_to_batch(const int* ptr, int B, int* batch, hipStream_t st) {
    if (B == 0) return hipSuccess;
    hipLaunchKernelGGL(ptr_to_batch, dim3(B), dim3(256), 0, st, ptr, B, batch);
    return hipGetLastError();
}

}  // namespace gn
