// graphnet_amd/csrc/nodes.hip — node definitions on the device (gfx950).
//
//   PercentileClusters (models/graphs/nodes/nodes.py:135-217, arithmetic of models/graphs/utils.py:12-172): the pulses of
//   an event become one node per distinct tuple of the cluster columns; every other column is summarised by percentiles.
//
//   pct_cluster_kernel   one workgroup per event.  C stable bitonic passes over 64-bit keys (column key << 32 | position),
//                        least significant cluster column (the FIRST of cluster_on) first, give the reference's lexsort
//                        order; cluster heads are flagged, a workgroup scan turns the flags into each pulse's cluster rank.
//                        Out (all in `work`): rank per pulse, first pulse and first sorted position per cluster, cluster
//                        count per event.
//   (launch_scan over the counts -> out_ptr)
//   pct_summary_kernel   one workgroup per (event, summarised column): sort (rank << 32 | value key), NaN last inside its
//                        cluster, then one thread per (cluster, percentile) does numpy's linear interpolation in fp64.
//
//   NodeAsDOMTimeSeries (nodes.py:220-306) is further down, on the same sort routine: dts_rows_kernel, dts_series_kernel.
//   IceMixNodes (nodes.py:309-453) is last and sorts nothing: imx_ptr_kernel, imx_nodes_kernel.
//
// Events of up to PCT_LDS_MAX pulses sort in LDS; larger ones run the same routine on their slice of `work` in global
// memory (still one workgroup per event, so __syncthreads() orders the steps; correct, not fast).
#include "launchers.hpp"

namespace gn {

constexpr int PCT_NT = 256;            // threads per workgroup
constexpr int PCT_LDS_MAX = 4096;      // 32 KB of keys + 16 KB of permutation
constexpr int PCT_CMAX = 8, PCT_SMAX = 32, PCT_PMAX = 16;
constexpr unsigned int PCT_NAN_KEY = 0xffffffffu;       // after +inf (0xff800000)
typedef unsigned long long u64;

struct PctArgs { int cl[PCT_CMAX]; int sm[PCT_SMAX]; double q[PCT_PMAX]; };

// order-preserving map of fp32 bits to unsigned
__device__ __forceinline__ unsigned int pct_ord(unsigned int b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
// cluster columns: -0.0 with +0.0, every NaN one key
__device__ __forceinline__ unsigned int pct_cluster_key(float v) {
    if (v != v) return PCT_NAN_KEY;
    if (v == 0.0f) return 0x80000000u;
    return pct_ord(__float_as_uint(v));
}
// summarised columns: the value's own bits (so that it can be read back from the key), every NaN one key
__device__ __forceinline__ unsigned int pct_value_key(float v) { return v != v ? PCT_NAN_KEY : pct_ord(__float_as_uint(v)); }
__device__ __forceinline__ float pct_key_value(unsigned int u) {
    return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// ascending bitonic sort of keys[0..P), P a power of two >= 2; ends with a barrier
template <typename KP>
__device__ __forceinline__ void pct_sort(KP keys, int P, int tid) {
    for (int kk = 2; kk <= P; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += PCT_NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const u64 a = keys[i], b = keys[l];
                if ((a > b) == ((i & kk) == 0)) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
}

__device__ __forceinline__ int pct_pow2(int n) {
    int P = 2;
    while (P < n) P <<= 1;
    return P;
}

// one stable pass: perm[0..n) reordered ascending by the cluster key of column `col`, ties in their present order
template <typename KP, typename IP>
__device__ __forceinline__ void pct_sort_pass(KP keys, IP perm, const float* __restrict__ x, long long ldx, int col, int lo, int n,
                                              int P, int tid) {
    for (int i = tid; i < P; i += PCT_NT)
        keys[i] = i < n ? ((u64)pct_cluster_key(x[(long long)(lo + perm[i]) * ldx + col]) << 32) | (unsigned int)i : ~0ull;
    __syncthreads();
    pct_sort(keys, P, tid);
    for (int i = tid; i < n; i += PCT_NT) keys[i] = (u64)(unsigned int)perm[(int)(keys[i] & 0xffffffffu)];
    __syncthreads();
    for (int i = tid; i < n; i += PCT_NT) perm[i] = (int)keys[i];
    __syncthreads();
}

template <typename KP, typename IP>
__device__ __forceinline__ void pct_cluster_event(
    KP keys, IP perm, int* part, const float* __restrict__ x, long long ldx, const PctArgs& a, int C, int lo, int n, int tid,
    int* __restrict__ rank, int* __restrict__ first, int* __restrict__ start, int* __restrict__ cnt_ev)
{
    const int P = pct_pow2(n);
    for (int i = tid; i < n; i += PCT_NT) perm[i] = i;
    __syncthreads();
    for (int c = 0; c < C; ++c) pct_sort_pass(keys, perm, x, ldx, a.cl[c], lo, n, P, tid);
    // head flags (into keys), then a scan over contiguous chunks
    for (int i = tid; i < n; i += PCT_NT) {
        bool head = i == 0;
        if (i > 0) {
            const float* r0 = x + (long long)(lo + perm[i - 1]) * ldx;
            const float* r1 = x + (long long)(lo + perm[i]) * ldx;
            for (int c = 0; c < C; ++c) head = head || pct_cluster_key(r0[a.cl[c]]) != pct_cluster_key(r1[a.cl[c]]);
        }
        keys[i] = head ? 1ull : 0ull;
    }
    __syncthreads();
    const int ipt = (n + PCT_NT - 1) / PCT_NT;
    const int i0 = min(tid * ipt, n), i1 = min(i0 + ipt, n);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += (int)keys[i];
    part[tid] = mine;
    __syncthreads();
    for (int o = 1; o < PCT_NT; o <<= 1) {                 // inclusive scan of the 256 chunk totals
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - mine;                            // heads before this chunk
    for (int i = i0; i < i1; ++i) {
        const int p = perm[i];
        if (keys[i]) { first[lo + run] = lo + p; start[lo + run] = i; ++run; }
        rank[lo + p] = run - 1;
    }
    if (tid == PCT_NT - 1) *cnt_ev = part[tid];
}

__global__ __launch_bounds__(PCT_NT) void pct_cluster_kernel(
    const float* __restrict__ x, long long ldx, PctArgs a, int C, const int* __restrict__ ptr, int N,
    int* __restrict__ rank, int* __restrict__ first, int* __restrict__ start, int* __restrict__ cnt,
    u64* __restrict__ gkeys, int* __restrict__ gperm)
{
    __shared__ u64 skeys[PCT_LDS_MAX];
    __shared__ int sperm[PCT_LDS_MAX];
    __shared__ int part[PCT_NT];
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int n = hi - lo;
    if (n <= 0) { if (tid == 0) cnt[ev] = 0; return; }
    if (n <= PCT_LDS_MAX) pct_cluster_event(skeys, sperm, part, x, ldx, a, C, lo, n, tid, rank, first, start, cnt + ev);
    else pct_cluster_event(gkeys + 2ll * lo, gperm + lo, part, x, ldx, a, C, lo, n, tid, rank, first, start, cnt + ev);
}

// numpy's linear method on the ascending non-NaN values keys[a0 .. a0 + m) of one cluster
template <typename KP>
__device__ __forceinline__ float pct_lerp(KP keys, int a0, int m, double q) {
#pragma clang fp contract(off)
    if (m <= 0) return __builtin_nanf("");
    const double h = (double)(m - 1) * q;
    const double fl = __builtin_floor(h);
    const int lo = (int)fl;
    const int hi = min(lo + 1, m - 1);
    const double g = h - fl;
    const double a = (double)pct_key_value((unsigned int)(keys[a0 + lo] & 0xffffffffu));
    const double b = (double)pct_key_value((unsigned int)(keys[a0 + hi] & 0xffffffffu));
    const double d = b - a;
    const double r = (g >= 0.5) ? b - d * (1.0 - g) : a + d * g;
    return (float)r;
}

template <typename KP>
__device__ __forceinline__ void pct_summary_column(
    KP keys, const float* __restrict__ x, long long ldx, int col, const PctArgs& a, int Pq, int lo, int n, int ncl, int tid,
    const int* __restrict__ rank, const int* __restrict__ start, float* __restrict__ o, long long ldo, long long rows_left)
{
    const int P = pct_pow2(n);
    for (int i = tid; i < P; i += PCT_NT)
        keys[i] = i < n ? ((u64)(unsigned int)rank[lo + i] << 32) | pct_value_key(x[(long long)(lo + i) * ldx + col]) : ~0ull;
    __syncthreads();
    pct_sort(keys, P, tid);
    for (int idx = tid; idx < ncl * Pq; idx += PCT_NT) {
        const int r = idx / Pq, p = idx - r * Pq;
        if (r >= rows_left) continue;
        const int s0 = start[lo + r], s1 = r + 1 < ncl ? start[lo + r + 1] : n;
        int l = s0, h = s1;                                 // first NaN of the segment
        while (l < h) {
            const int mid = (l + h) >> 1;
            if ((unsigned int)(keys[mid] & 0xffffffffu) == PCT_NAN_KEY) h = mid; else l = mid + 1;
        }
        o[(long long)r * ldo + p] = pct_lerp(keys, s0, l - s0, a.q[p]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(PCT_NT) void pct_summary_kernel(
    const float* __restrict__ x, long long ldx, PctArgs a, int C, int S, int Pq, int add_counts, const int* __restrict__ ptr, int N,
    const int* __restrict__ rank, const int* __restrict__ first, const int* __restrict__ start, const int* __restrict__ out_ptr,
    float* __restrict__ out, long long ldo, u64* __restrict__ gkeys)
{
    __shared__ u64 skeys[PCT_LDS_MAX];
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int n = hi - lo;
    if (n <= 0) return;
    const int ob = out_ptr[ev], ncl = out_ptr[ev + 1] - ob;
    const long long rows_left = (long long)N - ob;          // out has N rows: nothing is written past them
    float* o = out + (long long)ob * ldo;
    if (blockIdx.y == 0) {
        for (int idx = tid; idx < ncl * C; idx += PCT_NT) {
            const int r = idx / C, c = idx - r * C;
            if (r < rows_left) o[(long long)r * ldo + c] = x[(long long)first[lo + r] * ldx + a.cl[c]];
        }
        if (add_counts)
            for (int r = tid; r < ncl; r += PCT_NT) {
                const int count = (r + 1 < ncl ? start[lo + r + 1] : n) - start[lo + r];
                if (r < rows_left) o[(long long)r * ldo + C + S * Pq] = count == 1 ? 0.0f : (float)log10((double)count);
            }
    }
    if (n <= PCT_LDS_MAX) {
        const int s = (int)blockIdx.y;
        pct_summary_column(skeys, x, ldx, a.sm[s], a, Pq, lo, n, ncl, tid, rank, start, o + C + s * Pq, ldo, rows_left);
    } else if (blockIdx.y == 0) {
        for (int s = 0; s < S; ++s)
            pct_summary_column(gkeys + 2ll * lo, x, ldx, a.sm[s], a, Pq, lo, n, ncl, tid, rank, start, o + C + s * Pq, ldo,
                               rows_left);
    }
}

// work: [keys 4N + perm N ints, only if N > PCT_LDS_MAX][rank N][first N][start N][cnt B][scan tmp]
int percentile_lds_max() { return PCT_LDS_MAX; }
static long long pct_big_ints(int N) { return N > PCT_LDS_MAX ? 5ll * N : 0; }
static long long pct_scan_tmp(int B) { return ((long long)B + 2047) / 2048 + 1; }
long long percentile_work_ints(int B, int N) { return pct_big_ints(N) + 3ll * N + B + pct_scan_tmp(B); }

hipError_t launch_percentile_clusters(const float* x, long long ldx, int N, const int* ptr, int B, const int* cluster_cols, int C,
                                      const int* summ_cols, int S, const double* q, int P, int add_counts, float* out,
                                      long long ldo, int* out_ptr, int* work, hipStream_t st) {
    if (B == 0) return hipSuccess;
    if (N == 0) return hipMemsetAsync(out_ptr, 0, sizeof(int) * ((size_t)B + 1), st);
    PctArgs a;
    for (int i = 0; i < PCT_CMAX; ++i) a.cl[i] = i < C ? cluster_cols[i] : 0;
    for (int i = 0; i < PCT_SMAX; ++i) a.sm[i] = i < S ? summ_cols[i] : 0;
    for (int i = 0; i < PCT_PMAX; ++i) a.q[i] = i < P ? q[i] : 0.0;
    u64* gkeys = reinterpret_cast<u64*>(work);              // 8-byte aligned: the first thing in `work`
    int* gperm = work + 4ll * N;
    int* rank = work + pct_big_ints(N);
    int* first = rank + N;
    int* start = first + N;
    int* cnt = start + N;
    int* tmp = cnt + B;
    hipLaunchKernelGGL(pct_cluster_kernel, dim3((unsigned)B), dim3(PCT_NT), 0, st, x, ldx, a, C, ptr, N, rank, first, start, cnt,
                       gkeys, gperm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan(cnt, out_ptr, B, tmp, out_ptr + B, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pct_summary_kernel, dim3((unsigned)B, (unsigned)S), dim3(PCT_NT), 0, st, x, ldx, a, C, S, P, add_counts, ptr,
                       N, rank, first, start, out_ptr, out, ldo, gkeys);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
//   NodeAsDOMTimeSeries (models/graphs/nodes/nodes.py:220-306): the pulses of an event regrouped into one time series
//   per DOM.  Row count unchanged; the contract is in include/graphnet_amd.h (gn_dom_time_series).
//
//   dts_rows_kernel     one workgroup per event.  Minimum of the time column (NaN if any NaN), C + 1 stable passes (time,
//                       then the id columns, the first of id_cols first), head flags on the id tuples, a workgroup scan,
//                       then the permuted rows with the time shifted, the charge raised to 10^x and new_node_col.
//                       Into `work`: the batch row at which every series of the event starts, and the event's series count.
//   (launch_scan over the counts -> dom_ptr)
//   dts_series_kernel   series_ptr[dom_ptr[ev] + r] = start of series r of event ev;  series_ptr[M] = N.
struct DtsArgs { int id[PCT_CMAX]; };

template <typename KP, typename IP>
__device__ __forceinline__ void dts_event(
    KP keys, IP perm, int* part, const float* __restrict__ x, long long ldx, int F, const DtsArgs& a, int C, int time_col,
    int charge_col, int lo, int n, int tid, float* __restrict__ out, long long ldo, int* __restrict__ start,
    int* __restrict__ cnt_ev)
{
    const int P = pct_pow2(n);
    // smallest time in the order that puts -0.0 before +0.0; any NaN makes the whole column NaN (numpy's min)
    unsigned int kmin = 0xffffffffu;
    int anynan = 0;
    for (int i = tid; i < n; i += PCT_NT) {
        const float t = x[(long long)(lo + i) * ldx + time_col];
        if (t != t) anynan = 1; else kmin = min(kmin, pct_ord(__float_as_uint(t)));
        perm[i] = i;
    }
    part[tid] = (int)kmin;
    __syncthreads();
    for (int o = PCT_NT >> 1; o > 0; o >>= 1) {
        if (tid < o) part[tid] = (int)min((unsigned int)part[tid], (unsigned int)part[tid + o]);
        __syncthreads();
    }
    kmin = (unsigned int)part[0];
    __syncthreads();
    part[tid] = anynan;
    __syncthreads();
    for (int o = PCT_NT >> 1; o > 0; o >>= 1) {
        if (tid < o) part[tid] |= part[tid + o];
        __syncthreads();
    }
    anynan = part[0];
    __syncthreads();
    const float tmin = anynan ? __builtin_nanf("") : pct_key_value(kmin);

    pct_sort_pass(keys, perm, x, ldx, time_col, lo, n, P, tid);
    for (int c = 0; c < C; ++c) pct_sort_pass(keys, perm, x, ldx, a.id[c], lo, n, P, tid);

    for (int i = tid; i < n; i += PCT_NT) {                  // head flags (into keys)
        bool head = i == 0;
        if (i > 0) {
            const float* r0 = x + (long long)(lo + perm[i - 1]) * ldx;
            const float* r1 = x + (long long)(lo + perm[i]) * ldx;
            for (int c = 0; c < C; ++c) head = head || pct_cluster_key(r0[a.id[c]]) != pct_cluster_key(r1[a.id[c]]);
        }
        keys[i] = head ? 1ull : 0ull;
    }
    __syncthreads();
    const int ipt = (n + PCT_NT - 1) / PCT_NT;
    const int i0 = min(tid * ipt, n), i1 = min(i0 + ipt, n);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += (int)keys[i];
    part[tid] = mine;
    __syncthreads();
    for (int o = 1; o < PCT_NT; o <<= 1) {                 // inclusive scan of the 256 chunk totals
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - mine;                            // heads before this chunk
    for (int i = i0; i < i1; ++i)
        if (keys[i]) start[lo + run++] = lo + i;
    if (tid == PCT_NT - 1) *cnt_ev = part[tid];

    const int W = F + (charge_col < 0 ? 1 : 0) + 1;
    for (long long idx = tid; idx < (long long)n * W; idx += PCT_NT) {
        const int i = (int)(idx / W), c = (int)(idx - (long long)i * W);
        float v;
        if (c == W - 1) v = keys[i] ? 1.0f : 0.0f;
        else if (c >= F) v = 1.0f;                          // no charge column: 10^0
        else {
            v = x[(long long)(lo + perm[i]) * ldx + c];
            if (c == time_col) v = v - tmin;
            else if (c == charge_col) v = (float)pow(10.0, (double)v);
        }
        out[(long long)(lo + i) * ldo + c] = v;
    }
}

__global__ __launch_bounds__(PCT_NT) void dts_rows_kernel(
    const float* __restrict__ x, long long ldx, int F, DtsArgs a, int C, int time_col, int charge_col,
    const int* __restrict__ ptr, int N, float* __restrict__ out, long long ldo, int* __restrict__ start, int* __restrict__ cnt,
    u64* __restrict__ gkeys, int* __restrict__ gperm)
{
    __shared__ u64 skeys[PCT_LDS_MAX];
    __shared__ int sperm[PCT_LDS_MAX];
    __shared__ int part[PCT_NT];
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int n = hi - lo;
    if (n <= 0) { if (tid == 0) cnt[ev] = 0; return; }
    if (n <= PCT_LDS_MAX)
        dts_event(skeys, sperm, part, x, ldx, F, a, C, time_col, charge_col, lo, n, tid, out, ldo, start, cnt + ev);
    else
        dts_event(gkeys + 2ll * lo, gperm + lo, part, x, ldx, F, a, C, time_col, charge_col, lo, n, tid, out, ldo, start,
                  cnt + ev);
}

__global__ __launch_bounds__(PCT_NT) void dts_series_kernel(
    const int* __restrict__ ptr, int B, int N, const int* __restrict__ start, const int* __restrict__ dom_ptr,
    int* __restrict__ series_ptr)
{
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int s0 = dom_ptr[ev], ns = min(dom_ptr[ev + 1] - s0, hi - lo);
    for (int r = tid; r < ns; r += PCT_NT)
        if (s0 + r < N) series_ptr[s0 + r] = start[lo + r];
    if (ev == B - 1 && tid == 0) series_ptr[min(max(dom_ptr[B], 0), N)] = N;
}

// work: [keys 4N + perm N ints, only if N > PCT_LDS_MAX][start N][cnt B][scan tmp]
long long dom_time_series_work_ints(int B, int N) { return pct_big_ints(N) + (long long)N + B + pct_scan_tmp(B); }

hipError_t launch_dom_time_series(const float* x, long long ldx, int F, int N, const int* ptr, int B, const int* id_cols, int C,
                                  int time_col, int charge_col, float* out, long long ldo, int* series_ptr, int* dom_ptr,
                                  int* work, hipStream_t st) {
    if (B == 0) return series_ptr ? hipMemsetAsync(series_ptr, 0, sizeof(int), st) : hipSuccess;
    if (N == 0) {
        hipError_t e = hipMemsetAsync(dom_ptr, 0, sizeof(int) * ((size_t)B + 1), st);
        return e != hipSuccess ? e : hipMemsetAsync(series_ptr, 0, sizeof(int), st);
    }
    DtsArgs a;
    for (int i = 0; i < PCT_CMAX; ++i) a.id[i] = i < C ? id_cols[i] : 0;
    u64* gkeys = reinterpret_cast<u64*>(work);              // 8-byte aligned: the first thing in `work`
    int* gperm = work + 4ll * N;
    int* start = work + pct_big_ints(N);
    int* cnt = start + N;
    int* tmp = cnt + B;
    hipLaunchKernelGGL(dts_rows_kernel, dim3((unsigned)B), dim3(PCT_NT), 0, st, x, ldx, F, a, C, time_col, charge_col, ptr, N,
                       out, ldo, start, cnt, gkeys, gperm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_scan(cnt, dom_ptr, B, tmp, dom_ptr + B, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dts_series_kernel, dim3((unsigned)B), dim3(PCT_NT), 0, st, ptr, B, N, start, dom_ptr, series_ptr);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
//   IceMixNodes (models/graphs/nodes/nodes.py:309-453): every event cut to a uniformly random L of its pulses, kept in
//   pulse order, the hlc column flipped and two ice columns interpolated from a table.  The contract is in
//   include/graphnet_amd.h (gn_icemix_nodes).  No scratch in global memory, no limit on the size of an event.
//
//   imx_ptr_kernel      one workgroup: out_ptr = exclusive scan of min(n_b, L), straight from ptr (launch_scan would need
//                       a count array and its tmp, which this entry does not have).
//   imx_nodes_kernel    one workgroup per event.  n <= L: a coalesced row copy.  n > L: a radix select on the stateless
//                       hash (four passes of 8-bit digits over a 256-bin integer histogram, the hash recomputed each time)
//                       gives the L-th smallest key t and the number r of pulses with key t to keep; one pass in index
//                       order (chunks of 256, a workgroup scan of packed (below, equal) counts) ranks the kept pulses and
//                       writes ids; then the same row copy through ids.
constexpr int IMX_PT = 1024;
static_assert(PCT_NT == 256, "imx_nodes_kernel: one thread per histogram bin");

// inclusive scan of part[0..NT) in place; ends with a barrier
template <int NT>
__device__ __forceinline__ void imx_scan(int* part, int tid) {
    for (int o = 1; o < NT; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
}

__global__ __launch_bounds__(IMX_PT) void imx_ptr_kernel(const int* __restrict__ ptr, int B, int N, int L,
                                                         int* __restrict__ out_ptr)
{
    __shared__ int part[IMX_PT];
    const int tid = (int)threadIdx.x;
    int run = 0;
    for (int base = 0; base < B; base += IMX_PT) {
        const int b = base + tid;
        int c = 0;
        if (b < B) {
            const int hi = min(ptr[b + 1], N), lo = min(max(ptr[b], 0), hi);
            c = min(hi - lo, L);
        }
        part[tid] = c;
        __syncthreads();
        imx_scan<IMX_PT>(part, tid);
        if (b < B) out_ptr[b] = run + part[tid] - c;
        run += part[IMX_PT - 1];
        __syncthreads();
    }
    if (tid == 0) out_ptr[B] = run;
}

__device__ __forceinline__ unsigned int imx_key(unsigned int stream, unsigned int i, int shift) {
    return gn_mix32(stream ^ (i * 0x85EBCA77u)) >> shift;
}

// both ice columns of one pulse: linear interpolation in fp64, one rounding per operation, NaN outside the table
__device__ __forceinline__ void imx_ice(const double* tab, int T, float zf, float* sc, float* ab) {
#pragma clang fp contract(off)
    const double z = (double)zf;
    const double* zt = tab;
    if (!(z >= zt[0] && z <= zt[T - 1])) { *sc = *ab = __builtin_nanf(""); return; }
    int l = 0, h = T - 1;                                   // zt[l] <= z, and z < zt[h] or h == T - 1
    while (h - l > 1) {
        const int mid = (l + h) >> 1;
        if (zt[mid] <= z) l = mid; else h = mid;
    }
    const double dz = zt[l + 1] - zt[l], t = z - zt[l];
    const double* ys = tab + T;
    const double* ya = tab + 2 * T;
    const double ss = (ys[l + 1] - ys[l]) / dz, sa = (ya[l + 1] - ya[l]) / dz;
    const double ps = ss * t, pa = sa * t;
    *sc = (float)(ps + ys[l]);
    *ab = (float)(pa + ya[l]);
}

__global__ __launch_bounds__(PCT_NT) void imx_nodes_kernel(
    const float* __restrict__ x, long long ldx, int F, const int* __restrict__ ptr, int N, int L, int hlc_col, int z_col,
    const double* __restrict__ table, int T, unsigned int seed, const unsigned int* __restrict__ event_ids, int shift,
    const int* __restrict__ out_ptr, float* __restrict__ out, long long ldo, int* ids)
{
    extern __shared__ __attribute__((aligned(16))) double imx_lds[];       // [3T table][256 ints][2 ints]
    double* stab = imx_lds;
    int* part = reinterpret_cast<int*>(imx_lds + 3 * T);
    int* found = part + PCT_NT;
    const int ev = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int hi = min(ptr[ev + 1], N), lo = min(max(ptr[ev], 0), hi);
    const int n = hi - lo;
    if (n <= 0) return;
    const int ob = out_ptr[ev];
    const int m = min(min(n, L), N - ob);                   // never more kept rows than pulses: nothing past row N - 1
    for (int i = tid; i < 3 * T; i += PCT_NT) stab[i] = table[i];
    if (n <= L) {
        for (int r = tid; r < m; r += PCT_NT) ids[ob + r] = lo + r;
    } else {
        const unsigned int stream = gn_mix32(seed ^ ((event_ids ? event_ids[ev] : (unsigned int)ev) * 0x9E3779B1u));
        unsigned int prefix = 0, mask = 0;
        int r = L;                                          // the r-th smallest (from 1) among the keys that match prefix
        for (int dshift = 24; dshift >= 0; dshift -= 8) {
            part[tid] = 0;
            __syncthreads();
            for (int i = tid; i < n; i += PCT_NT) {
                const unsigned int h = imx_key(stream, (unsigned int)i, shift);
                if ((h & mask) == prefix) atomicAdd(&part[(h >> dshift) & 255u], 1);
            }
            __syncthreads();
            const int mine = part[tid];
            imx_scan<PCT_NT>(part, tid);
            const int below = part[tid] - mine;
            if (below < r && r <= part[tid]) { found[0] = tid; found[1] = below; }
            __syncthreads();
            prefix |= (unsigned int)found[0] << dshift;
            mask |= 0xffu << dshift;
            r -= found[1];
            __syncthreads();
        }
        // prefix: the L-th smallest key; kept: every key below it and the r lowest-index pulses that have it
        int lt_run = 0, eq_run = 0;
        for (int base = 0; base < n; base += PCT_NT) {
            const int i = base + tid;
            int lt = 0, eq = 0;
            if (i < n) {
                const unsigned int h = imx_key(stream, (unsigned int)i, shift);
                lt = h < prefix; eq = h == prefix;
            }
            const int mine = lt | (eq << 16);               // at most 256 of either in a chunk
            part[tid] = mine;
            __syncthreads();
            imx_scan<PCT_NT>(part, tid);
            const int before = part[tid] - mine;
            const int lt_before = lt_run + (before & 0xffff), eq_before = eq_run + (before >> 16);
            if (lt || (eq && eq_before < r)) {
                const int pos = lt_before + min(eq_before, r);
                if (pos < m) ids[ob + pos] = lo + i;
            }
            const int total = part[PCT_NT - 1];
            lt_run += total & 0xffff; eq_run += total >> 16;
            __syncthreads();
        }
    }
    __syncthreads();                                        // the table and this event's ids
    for (long long idx = tid; idx < (long long)m * F; idx += PCT_NT) {
        const int r = (int)(idx / F), c = (int)(idx - (long long)r * F);
        const int src = n <= L ? lo + r : ids[ob + r];
        float v = x[(long long)src * ldx + c];
        if (c == hlc_col) v = v == 0.0f ? 1.0f : 0.0f;
        out[(long long)(ob + r) * ldo + c] = v;
    }
    if (z_col >= 0)
        for (int r = tid; r < m; r += PCT_NT) {
            const int src = n <= L ? lo + r : ids[ob + r];
            float* o = out + (long long)(ob + r) * ldo + F;
            imx_ice(stab, T, x[(long long)src * ldx + z_col], o, o + 1);
        }
}

hipError_t launch_icemix_nodes(const float* x, long long ldx, int F, int N, const int* ptr, int B, int L, int hlc_col, int z_col,
                               const double* table, int T, unsigned int seed, const unsigned int* event_ids, int key_bits,
                               float* out, long long ldo, int* out_ptr, int* ids, hipStream_t st) {
    if (B == 0) return hipSuccess;
    if (N == 0) return hipMemsetAsync(out_ptr, 0, sizeof(int) * ((size_t)B + 1), st);
    hipLaunchKernelGGL(imx_ptr_kernel, dim3(1), dim3(IMX_PT), 0, st, ptr, B, N, L, out_ptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int Tl = z_col >= 0 ? T : 0;
    const size_t lds = sizeof(double) * 3 * (size_t)Tl + sizeof(int) * (PCT_NT + 2);
    hipLaunchKernelGGL(imx_nodes_kernel, dim3((unsigned)B), dim3(PCT_NT), lds, st, x, ldx, F, ptr, N, L, hlc_col, z_col, table,
                       Tl, seed, event_ids, 32 - key_bits, out_ptr, out, ldo, ids);
    return hipGetLastError();
}

}  // namespace gn
