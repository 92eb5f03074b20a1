// graphnet_amd/csrc/step.hip — one C entry for the whole DynEdge backbone pass (gn_dynedge_fwd / gn_dynedge_bwd).
//
// Replaces, as ONE host call each, what DynEdge.forward (models/gnn/dynedge.py:295-349: global variables, 4 x
// DynEdgeConv incl. the k-NN re-clustering of models/components/layers.py:55-69, skip-cat, post-processing MLP,
// global pooling) and its autograd backward enqueue: ~110 kernel launches that the per-op path of graphnet_amd/gnn.py
// issues through ~110 ctypes crossings plus as many torch allocations.  The reference's users train at batch 16 - 256
// (examples/04_training/01_train_dynedge.py:223), where a step is a few hundred microseconds of kernels: there the host
// IS the step time.  Same kernels, same arguments, same order as the per-op path => bit-identical results (tested).
//
// Memory: the caller owns everything.  `wws` (persistent, zero-initialised ONCE by the caller) holds the packed operand
// copies of the weights - only their real blocks are rewritten each step, the pads stay zero; `ws` (per step) holds
// every tensor the forward leaves for the backward at offsets that are a pure function of the descriptor; `bws` is the
// backward's scratch.  Nothing here allocates, copies to the host or synchronises.
#include "../../include/graphnet_amd.h"
#include "launchers.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace gn {
int device_cus();

// ---- operand copies described by kernel ARGUMENTS (no descriptor table in device memory to keep in sync) -----------
// dst[r * d_pitch + c] = src[r * s_row + c * s_col] - (src2 ? src2[same] : 0), r < rows, c < cols; dst fp32 or bf16
struct PackItem { const float* src; const float* src2; void* dst; long long s_row, s_col, d_pitch, rows, cols; int lowp; int pad; };
constexpr int PACK_MAX = 28;
struct PackArgs { PackItem it[PACK_MAX]; };
__global__ __launch_bounds__(256) void pack_args_kernel(PackArgs a) {
    const PackItem& d = a.it[blockIdx.y];
    const long long total = d.rows * d.cols;
    const bool by_src = d.s_row == 1 && d.s_col != 1;      // a transpose: walk the source contiguously
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = by_src ? i % d.rows : i / d.cols, c = by_src ? i / d.rows : i % d.cols;
        float v = d.src[r * d.s_row + c * d.s_col];
        if (d.src2) v -= d.src2[r * d.s_row + c * d.s_col];
        if (d.lowp) reinterpret_cast<__bf16*>(d.dst)[r * d.d_pitch + c] = (__bf16)v;
        else reinterpret_cast<float*>(d.dst)[r * d.d_pitch + c] = v;
    }
}
struct Packer {
    PackArgs args;
    int n = 0;
    hipStream_t st;
    hipError_t err = hipSuccess;
    explicit Packer(hipStream_t s) : st(s) {}
    void flush() {
        if (n > 0 && err == hipSuccess) {
            hipLaunchKernelGGL(pack_args_kernel, dim3(32, n), dim3(256), 0, st, args);
            err = hipGetLastError();
        }
        n = 0;
    }
    void add(void* dst, long long d_pitch, int lowp, const float* src, long long s_row, long long s_col, long long rows,
             long long cols, const float* src2 = nullptr) {
        if (rows <= 0 || cols <= 0) return;
        if (n == PACK_MAX) flush();
        args.it[n++] = PackItem{src, src2, dst, s_row, s_col, d_pitch, rows, cols, lowp, 0};
    }
};

// ---- optional per-op HIP events (bench.py's live kernel durations; off by default: no events, no cost) ---------------
struct StepTimer { std::string name; hipEvent_t a, b; };
static std::vector<StepTimer> g_timers;
static bool g_timers_on = false;
struct Timed {
    hipStream_t st;
    bool on;
    size_t idx = 0;
    Timed(hipStream_t s, const char* name, int a = -1, int b = -1) : st(s), on(g_timers_on) {
        if (!on) return;
        char buf[96];
        if (a >= 0) std::snprintf(buf, sizeof(buf), "%s[%dx%d]", name, a, b);
        else std::snprintf(buf, sizeof(buf), "%s", name);
        StepTimer t;
        t.name = buf;
        (void)hipEventCreate(&t.a);
        (void)hipEventCreate(&t.b);
        (void)hipEventRecord(t.a, st);
        idx = g_timers.size();
        g_timers.push_back(t);
    }
    ~Timed() { if (on) (void)hipEventRecord(g_timers[idx].b, st); }
};

static inline long long up(long long v, long long m) { return (v + m - 1) / m * m; }

// ---- arena: offsets are a pure function of the descriptor, so forward and backward agree on them -------------------
struct Arena {
    unsigned char* base;
    long long off = 0;
    explicit Arena(void* b) : base(reinterpret_cast<unsigned char*>(b)) {}
    template <typename T> T* take(long long count) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += up((count > 0 ? count : 1) * (long long)sizeof(T), 256);
        return p;
    }
    void* bytes(long long n) { return take<unsigned char>(n); }
};

struct Table {             // one layer's graph
    int* nbr; int* ovf; int* ovf_pos; int* oc; int* os; int* cnt; int K; bool event_local;
    EdgeGraph graph(int N) const { EdgeGraph g; g.nbr = nbr; g.ovf_centre = oc; g.ovf_src = os; g.ovf_cnt = cnt; g.N = N; g.K = K; return g; }
};

struct Shapes {
    int mode, es /* bytes per activation element */, unit, ku, N, B, F, G, F0, ld0, k, nconv, npost, npool;
    int Fin[GN_DYNEDGE_MAX_CONV], H1[GN_DYNEDGE_MAX_CONV], H1p[GN_DYNEDGE_MAX_CONV], H2[GN_DYNEDGE_MAX_CONV];
    int P[GN_DYNEDGE_MAX_POST], Pr[GN_DYNEDGE_MAX_POST];
    int seg_w[GN_DYNEDGE_MAX_CONV + 1], seg_pad[GN_DYNEDGE_MAX_CONV + 1], seg_off[GN_DYNEDGE_MAX_CONV + 2];   // skip-cat segments
    bool lowp;
    int kw(int w) const { return (int)up(w, unit); }
};
static bool make_shapes(const GnDynEdgeDesc& d, Shapes& s, const char** why) {
    *why = nullptr;
    if (d.struct_bytes != (int32_t)sizeof(GnDynEdgeDesc)) { *why = "struct_bytes != sizeof(GnDynEdgeDesc): header / library mismatch"; return false; }
    if (d.mode != 0 && d.mode != 1) { *why = "mode"; return false; }
    if (d.N < 1 || d.B < 1 || d.F < 4 || d.F > 32) { *why = "need N >= 1, B >= 1, 4 <= F <= 32"; return false; }
    if (d.G != 0 && d.G != d.F + 5) { *why = "G must be 0 or F + 5"; return false; }
    if (d.k < 1 || d.k > 32) { *why = "1 <= k <= 32"; return false; }
    if (d.nconv < 1 || d.nconv > GN_DYNEDGE_MAX_CONV || d.npost < 1 || d.npost > GN_DYNEDGE_MAX_POST) { *why = "layer counts"; return false; }
    if (d.npool < 1 || d.npool > 4) { *why = "1..4 pooling schemes (node-level output runs on the per-op path)"; return false; }
    if (d.n_knn_cols < 1 || d.n_knn_cols > 8) { *why = "1..8 k-NN columns"; return false; }
    s.mode = d.mode; s.lowp = d.mode == 1; s.es = s.lowp ? 2 : 4; s.unit = s.lowp ? 8 : 4; s.ku = s.lowp ? 64 : 32;
    s.N = d.N; s.B = d.B; s.F = d.F; s.G = d.G; s.F0 = d.F + d.G; s.ld0 = (int)up(s.F0, 32); s.k = d.k;
    s.nconv = d.nconv; s.npost = d.npost; s.npool = d.npool;
    int fin = s.F0;
    s.seg_w[0] = s.F0;
    for (int l = 0; l < d.nconv; ++l) {
        if (d.H1[l] < 1 || d.H2[l] < 1 || d.H2[l] % 8) { *why = "conv widths: H2 must be a multiple of 8"; return false; }
        s.Fin[l] = fin; s.H1[l] = d.H1[l]; s.H1p[l] = (int)up(d.H1[l], 32); s.H2[l] = d.H2[l];
        fin = d.H2[l];
        s.seg_w[l + 1] = d.H2[l];
        for (int c = 0; c < d.n_knn_cols; ++c) if (l + 1 < d.nconv && (d.knn_cols[c] < 0 || d.knn_cols[c] >= d.H2[l])) { *why = "k-NN column out of range"; return false; }
    }
    s.seg_off[0] = 0;
    for (int i = 0; i <= d.nconv; ++i) { s.seg_pad[i] = (int)up(s.seg_w[i], 32); s.seg_off[i + 1] = s.seg_off[i] + s.seg_pad[i]; }
    if (d.nconv + 1 > MAXSEG) { *why = "at most 5 conv layers (6 skip-cat segments)"; return false; }
    for (int t = 0; t < d.npost; ++t) {
        if (d.P[t] < 1) { *why = "post widths"; return false; }
        s.P[t] = d.P[t]; s.Pr[t] = (int)up(d.P[t], 8);
    }
    return true;
}

struct FwdBufs {
    int* plan; int* scan_tmp; void* knn_ws;
    Table tab[GN_DYNEDGE_MAX_CONV];
    void* x0; void* PQ[GN_DYNEDGE_MAX_CONV]; void* out[GN_DYNEDGE_MAX_CONV]; void* saved[GN_DYNEDGE_MAX_CONV];
    float* coords[GN_DYNEDGE_MAX_CONV];
    void* y[GN_DYNEDGE_MAX_POST];
    int* amin; int* amax; void* evscratch;
    long long total;
};
static void layout_fwd(const GnDynEdgeDesc& d, const Shapes& s, void* base, FwdBufs& f) {
    Arena a(base);
    const long long N = s.N;
    f.plan = a.take<int>(s.B + 2 + N / 64 + s.B);
    f.scan_tmp = a.take<int>(gn_scan_tmp_ints(N));
    f.knn_ws = (s.B > 0 && N >= 512LL * s.B) ? a.bytes(knn_ws_bytes(s.B, s.N, 8)) : nullptr;      // large events: sorted sweep (first graph)
    for (int l = 0; l < s.nconv; ++l) {
        Table& t = f.tab[l];
        if (l == 0 && d.nbr0) {
            t.nbr = const_cast<int*>(d.nbr0); t.ovf = const_cast<int*>(d.ovf0); t.ovf_pos = const_cast<int*>(d.ovf0_pos);
            t.oc = const_cast<int*>(d.ovf0_centre); t.os = const_cast<int*>(d.ovf0_src); t.cnt = const_cast<int*>(d.ovf0_cnt);
            t.K = d.K0; t.event_local = d.event_local0 != 0;
            continue;
        }
        t.K = s.k; t.event_local = true;
        t.nbr = a.take<int>(N * s.k);
        if (d.strict) { t.ovf = t.ovf_pos = t.oc = t.os = t.cnt = nullptr; }
        else { t.ovf = a.take<int>(N); t.ovf_pos = a.take<int>(N); t.oc = a.take<int>(N); t.os = a.take<int>(N); t.cnt = a.take<int>(1); }
    }
    f.x0 = a.bytes(N * s.ld0 * s.es);
    for (int l = 0; l < s.nconv; ++l) {
        f.PQ[l] = a.bytes(N * 2 * s.H1p[l] * s.es);
        f.out[l] = a.bytes(N * s.H2[l] * s.es);
        f.saved[l] = a.bytes(saved_layout(N, edge_slots(f.tab[l].K), s.H1p[l], s.H2[l]).total);
        f.coords[l] = (s.lowp && l + 1 < s.nconv) ? a.take<float>(N * 8) : nullptr;
    }
    for (int t = 0; t < s.npost; ++t) f.y[t] = a.bytes(N * s.Pr[t] * ((s.lowp && t + 1 < s.npost) ? 2 : 4));
    f.amin = a.take<int>((long long)s.B * s.P[s.npost - 1]);
    f.amax = a.take<int>((long long)s.B * s.P[s.npost - 1]);
    {   // per-event reductions of a batch of few huge events run in slices (pool.hip / graph.hip): their scratch
        const long long e1 = globals_scratch_bytes(s.B, s.N), e2 = pool_scratch_bytes(s.B, s.N, s.P[s.npost - 1]);
        f.evscratch = a.bytes(e1 > e2 ? e1 : e2);
    }
    f.total = a.off;
}

struct WBufs {   // packed operand copies of the weights (element type T = the mode's operand type, biases fp32)
    void* Wpq[GN_DYNEDGE_MAX_CONV]; float* bpq[GN_DYNEDGE_MAX_CONV]; void* W2p[GN_DYNEDGE_MAX_CONV]; void* W2T[GN_DYNEDGE_MAX_CONV];
    void* WpqT[GN_DYNEDGE_MAX_CONV];
    void* post[GN_DYNEDGE_MAX_POST]; void* postT[GN_DYNEDGE_MAX_POST]; void* catT;
    int post_kp[GN_DYNEDGE_MAX_POST];
    long long total;
};
static void layout_w(const Shapes& s, void* base, WBufs& w) {
    Arena a(base);
    for (int l = 0; l < s.nconv; ++l) {
        w.Wpq[l] = a.bytes(up(2 * s.H1p[l], 128) * up(s.Fin[l], s.ku) * s.es);
        w.bpq[l] = a.take<float>(2 * s.H1p[l]);
        w.W2p[l] = a.bytes(up(s.H2[l], 128) * up(s.H1[l], 32) * s.es);
        w.W2T[l] = a.bytes(up(s.H1[l], 128) * up(s.H2[l], 32) * s.es);
        w.WpqT[l] = l > 0 ? a.bytes(up(s.Fin[l], 128) * up(2 * s.H1p[l], s.ku) * s.es) : nullptr;
    }
    for (int t = 0; t < s.npost; ++t) {
        int kp = 0;
        if (t == 0) for (int i = 0; i <= s.nconv; ++i) kp += (int)up(s.seg_w[i], s.ku);
        else kp = (int)up(s.P[t - 1], s.ku);
        w.post_kp[t] = kp;
        w.post[t] = a.bytes(up(s.P[t], 128) * kp * s.es);
        w.postT[t] = t > 0 ? a.bytes(up(s.P[t - 1], 128) * up(s.P[t], s.ku) * s.es) : nullptr;
    }
    w.catT = a.bytes(up(s.seg_off[s.nconv + 1] - s.seg_off[1], 128) * up(s.P[0], s.ku) * s.es);
    w.total = a.off;
}

struct BwdBufs {
    void* dZ[2]; void* dXcat; void* dPQ; void* dpre; void* dpre_ovf; void* plan;
    float* slab; float* dbp; float* dWtmp; float* dbtmp;
    int* rev_ptr; int* rev_rows; int* ev; int* scratch; int* hubs; int* tmp; int* pairs;
    long long total;
};
static long long max_ll(long long a, long long b) { return a > b ? a : b; }
static void layout_bwd(const GnDynEdgeDesc& d, const Shapes& s, const FwdBufs& f, void* base, BwdBufs& b) {
    Arena a(base);
    const long long N = s.N;
    int prmax = 0;
    for (int t = 0; t < s.npost; ++t) prmax = s.Pr[t] > prmax ? s.Pr[t] : prmax;
    b.dZ[0] = a.bytes(N * prmax * s.es);
    b.dZ[1] = a.bytes(N * prmax * s.es);
    b.dXcat = a.bytes(N * s.seg_off[s.nconv + 1] * s.es);
    long long dpq = 0, dpre = 0, dovf = 0, plan = 0, slab = 0, dbp = 0, dwt = 0, dbt = 0, rows_max = 0, kmax = 1;
    for (int l = 0; l < s.nconv; ++l) {
        const int K = f.tab[l].K, S_ = edge_slots(K);
        const long long rows = N * S_ + N;
        dpq = max_ll(dpq, N * 2 * s.H1p[l] * s.es);
        dpre = max_ll(dpre, rows * s.H1p[l] * s.es);
        if (dpre_compact_supported(s.mode, K, s.H1p[l], s.H1[l], s.H2[l])) {     // compact stream + dense overflow rows + plan
            dpre = max_ll(dpre, dpre_compact_bytes(s.N, K, s.H1p[l]));
            dovf = max_ll(dovf, N * s.H1p[l] * s.es);
            plan = max_ll(plan, dpre_plan_layout(s.N, K, nullptr).total);
        }
        const int nslab = edge_dw2_slabs(s.mode, s.N, K, s.H1p[l], s.H2[l]);
        slab = max_ll(slab, (long long)nslab * s.H2[l] * s.H1[l]);
        dbp = max_ll(dbp, (long long)nslab * s.H2[l]);
        const int wk = s.kw(s.Fin[l]);
        const int parts = gemm_tn_parts(s.mode, s.N, 2 * s.H1p[l], &wk, 1);
        slab = max_ll(slab, (long long)parts * 2 * s.H1p[l] * wk);
        dbp = max_ll(dbp, (long long)max_ll(parts, colsum_blocks(s.N)) * 2 * s.H1p[l]);
        dwt += (long long)2 * s.H1p[l] * wk;          // one slice per use: all pad-dropping copies go in ONE launch at the end
        dbt += 2 * s.H1p[l];
        rows_max = max_ll(rows_max, N * K + N);
        kmax = max_ll(kmax, K);
    }
    for (int t = 0; t < s.npost; ++t) {
        int widths[MAXSEG], nseg = 0, ktot = 0;
        if (t == 0) for (int i = 0; i <= s.nconv; ++i) { widths[nseg++] = s.kw(s.seg_w[i]); ktot += widths[nseg - 1]; }
        else { widths[nseg++] = s.kw(s.P[t - 1]); ktot = widths[0]; }
        const int parts = gemm_tn_parts(s.mode, s.N, s.P[t], widths, nseg);
        slab = max_ll(slab, (long long)parts * s.P[t] * ktot);
        dbp = max_ll(dbp, (long long)max_ll(parts, colsum_blocks(s.N)) * s.P[t]);
        dwt += (long long)s.P[t] * ktot;
    }
    b.dPQ = a.bytes(dpq);
    b.dpre = a.bytes(dpre);
    b.dpre_ovf = a.bytes(dovf);
    b.plan = a.bytes(plan);
    b.slab = a.take<float>(slab);
    b.dbp = a.take<float>(dbp);
    b.dWtmp = a.take<float>(dwt);
    b.dbtmp = a.take<float>(dbt);
    const int G = s.B * rev_event_slices(s.B);
    b.rev_ptr = a.take<int>(N + 1);
    b.rev_rows = a.take<int>(rows_max);
    b.ev = a.take<int>(2 * ((long long)G + 1));
    b.scratch = a.take<int>(N);
    b.pairs = rev_pairs_ints(s.B, s.N, (int)kmax) > 0 ? a.take<int>(rev_pairs_ints(s.B, s.N, (int)kmax)) : nullptr;
    b.hubs = a.take<int>(N);
    b.tmp = a.take<int>(max_ll(gn_scan_tmp_ints(G > 0 ? G : 1), gn_scan_tmp_ints(N)) + 1);
    b.total = a.off;
    (void)d;
}

static Segs one_seg(const void* p, long long ld, int width, int ku) {
    Segs s;
    std::memset(&s, 0, sizeof(s));
    s.nseg = 1; s.p[0] = p; s.ld[0] = ld; s.width[0] = width; s.kpad[0] = (int)up(width, ku);
    return s;
}
static Epi epi(const float* bias = nullptr, int relu = 0, int accum = 0, const void* gate = nullptr, long long ldgate = 0, int gate_lowp = 0) {
    Epi e;
    e.bias = bias; e.gate = gate; e.ldgate = ldgate; e.relu = relu; e.accum = accum; e.gate_lowp = gate_lowp;
    return e;
}

#define GN_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return e__; } while (0)

// detector: the graph on the input coordinates (a DOM's pulses coincide: the sorted sweep of large events pays, 2.5x at 10^4
// pulses per event); the graphs on learned coordinates are scanned exhaustively (the sweep measured slower there)
static hipError_t build_graph(const Shapes& s, const GnDynEdgeDesc& d, const FwdBufs& f, Table& t, const float* x, long long ldx,
                              const int* cols, int ncols, bool detector, hipStream_t st) {
    {
        Timed tm(st, "knn_graph");
        GN_TRY(launch_knn(x, ldx, cols, ncols, d.ptr, f.plan, s.B, s.N, s.k, d.strict, t.nbr, t.ovf, detector ? f.knn_ws : nullptr, st));
    }
    if (!d.strict) GN_TRY(launch_ovf_compact(t.ovf, s.N, t.ovf_pos, f.scan_tmp, t.oc, t.os, t.cnt, st));
    return hipSuccess;
}

static hipError_t dynedge_fwd(const GnDynEdgeDesc& d, const Shapes& s, float* gv, float* out) {
    hipStream_t st = reinterpret_cast<hipStream_t>(d.stream);
    FwdBufs f;
    layout_fwd(d, s, d.ws, f);
    WBufs w;
    layout_w(s, d.wws, w);
    const int N = s.N, mode = s.mode, lowp = s.lowp ? 1 : 0;
    GN_TRY(launch_knn_plan(d.ptr, s.B, f.plan, st));
    if (!d.nbr0) GN_TRY(build_graph(s, d, f, f.tab[0], d.x, d.ldx, d.graph_cols, d.n_graph_cols, true, st));
    {
        Timed tm(st, "graph_globals");
        GN_TRY(launch_globals(d.x, d.ldx, s.F, d.ptr, s.B, f.tab[0].nbr, f.tab[0].ovf, f.tab[0].K, d.n_pulses, gv, st, f.evscratch, s.N));
    }
    GN_TRY(launch_concat_globals(d.x, d.ldx, s.F, s.G ? gv : d.x, s.G, d.batch, N, f.x0, s.ld0, lowp, st));
    // ---- operand copies of the weights the forward consumes: one launch
    {
        Packer pk(st);
        for (int l = 0; l < s.nconv; ++l) {
            const int Fin = s.Fin[l], H1 = s.H1[l], H1p = s.H1p[l];
            const long long ldw = 2LL * Fin, kp = up(Fin, s.ku);          // W1 is [H1, 2 Fin] = [Wa | Wb]
            unsigned char* wpq = reinterpret_cast<unsigned char*>(w.Wpq[l]);
            pk.add(wpq, kp, lowp, d.W1[l], ldw, 1, H1, Fin, d.W1[l] + Fin);                        // rows 0..H1: Wa - Wb
            pk.add(wpq + (long long)H1p * kp * s.es, kp, lowp, d.W1[l] + Fin, ldw, 1, H1, Fin);   // rows H1p..: Wb
            pk.add(w.bpq[l], 2 * H1p, 0, d.b1[l], H1, 1, 1, H1);
            pk.add(w.W2p[l], up(H1, 32), lowp, d.W2[l], H1, 1, s.H2[l], H1);
        }
        for (int t = 0; t < s.npost; ++t) {
            long long ldw = s.P[t > 0 ? t - 1 : 0];              // row pitch of Wp[t] = its input width
            if (t == 0) { ldw = 0; for (int i = 0; i <= s.nconv; ++i) ldw += s.seg_w[i]; }
            if (t == 0) {
                long long off = 0, offp = 0;
                for (int i = 0; i <= s.nconv; ++i) {
                    pk.add(reinterpret_cast<unsigned char*>(w.post[t]) + offp * s.es, w.post_kp[t], lowp, d.Wp[t] + off, ldw, 1, s.P[t], s.seg_w[i]);
                    off += s.seg_w[i];
                    offp += up(s.seg_w[i], s.ku);
                }
            } else {
                pk.add(w.post[t], w.post_kp[t], lowp, d.Wp[t], ldw, 1, s.P[t], s.P[t - 1]);
            }
        }
        pk.flush();
        GN_TRY(pk.err);
    }
    // ---- DynEdgeConv layers
    const void* xin = f.x0;
    long long ldin = s.ld0;
    int idcols[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    for (int l = 0; l < s.nconv; ++l) {
        const int Fin = s.Fin[l], H1 = s.H1[l], H1p = s.H1p[l], H2 = s.H2[l];
        {
            Timed tm(st, "linear_fwd", s.kw(Fin), 2 * H1p);
            GN_TRY(launch_gemm_nt(mode, one_seg(xin, ldin, s.kw(Fin), s.ku), lowp, N, w.Wpq[l], (int)up(Fin, s.ku), (int)up(2 * H1p, 128),
                                  2 * H1p, epi(w.bpq[l]), f.PQ[l], 2 * H1p, lowp, st));
        }
        const bool more = l + 1 < s.nconv;
        {
            Timed tm(st, "edgeconv_fwd", H1p, H2);
            GN_TRY(launch_edge_fwd(mode, f.tab[l].graph(N), f.PQ[l], H1p, H1, w.W2p[l], d.b2[l], H2, f.out[l], H2,
                                   (more && s.lowp) ? f.coords[l] : nullptr, d.knn_cols, (more && s.lowp) ? d.n_knn_cols : 0, f.saved[l], st));
        }
        if (more) {
            if (s.lowp) GN_TRY(build_graph(s, d, f, f.tab[l + 1], f.coords[l], 8, idcols, d.n_knn_cols, false, st));
            else GN_TRY(build_graph(s, d, f, f.tab[l + 1], reinterpret_cast<const float*>(f.out[l]), H2, d.knn_cols, d.n_knn_cols, false, st));
        }
        xin = f.out[l];
        ldin = H2;
    }
    // ---- post-processing MLP on the skip-cat (never materialised: one K segment per skip tensor)
    for (int t = 0; t < s.npost; ++t) {
        Segs a;
        std::memset(&a, 0, sizeof(a));
        if (t == 0) {
            a.nseg = s.nconv + 1;
            for (int i = 0; i <= s.nconv; ++i) {
                a.p[i] = i == 0 ? f.x0 : f.out[i - 1];
                a.ld[i] = i == 0 ? s.ld0 : s.H2[i - 1];
                a.width[i] = s.kw(s.seg_w[i]);
                a.kpad[i] = (int)up(a.width[i], s.ku);
            }
        } else {
            a = one_seg(f.y[t - 1], s.Pr[t - 1], s.kw(s.P[t - 1]), s.ku);
        }
        const int olp = (s.lowp && t + 1 < s.npost) ? 1 : 0;
        if (s.Pr[t] != s.P[t])         // pad columns of the output: zero (what the per-op path does with out[:, n_real:].zero_())
            GN_TRY(hipMemset2DAsync(reinterpret_cast<unsigned char*>(f.y[t]) + (long long)s.P[t] * (olp ? 2 : 4), (size_t)s.Pr[t] * (olp ? 2 : 4), 0,
                                    (size_t)(s.Pr[t] - s.P[t]) * (olp ? 2 : 4), (size_t)N, st));
        int ksum = 0;
        for (int i = 0; i < a.nseg; ++i) ksum += a.width[i];
        Timed tm(st, "linear_fwd", ksum, s.P[t]);
        GN_TRY(launch_gemm_nt(mode, a, lowp, N, w.post[t], w.post_kp[t], (int)up(s.P[t], 128), s.P[t], epi(d.bp[t], 1), f.y[t], s.Pr[t], olp, st));
    }
    {
        Timed tm(st, "segment_pool_fwd");
        const int last = s.npost - 1;
        GN_TRY(launch_pool_fwd(reinterpret_cast<const float*>(f.y[last]), s.Pr[last], s.P[last], d.ptr, s.B, s.N, d.pool_codes, s.npool, out, f.amin, f.amax, st, f.evscratch));
    }
    return hipSuccess;
}

static hipError_t build_reverse(const Shapes& s, const GnDynEdgeDesc& d, const Table& t, const BwdBufs& b, const int** hubs,
                                const int** nhubs, hipStream_t st) {
    Timed tm(st, "rev_build");
    const int S_ = edge_slots(t.K);
    if (t.event_local && (t.ovf == nullptr || t.ovf_pos != nullptr)) {
        const int G = s.B * rev_event_slices(s.B);
        int* nh = b.tmp + gn_scan_tmp_ints(G > 0 ? G : 1);
        GN_TRY(launch_rev_build_events(t.nbr, s.N, t.K, S_, t.ovf, t.ovf_pos, d.ptr, s.B, b.rev_ptr, b.rev_rows, b.ev, b.scratch, b.hubs, nh, b.tmp,
                                       b.pairs, st));
        *hubs = b.hubs; *nhubs = nh;
        return hipSuccess;
    }
    GN_TRY(launch_rev_build(t.nbr, s.N, t.K, S_, t.os, t.cnt, b.rev_ptr, b.scratch, b.tmp, b.rev_rows, st));
    *hubs = b.scratch; *nhubs = b.tmp;          // hub list / its length, left there by the global build
    return hipSuccess;
}

static hipError_t dynedge_bwd(const GnDynEdgeDesc& d, const Shapes& s, const float* gout, void* bws, const GnDynEdgeGrads& gr) {
    hipStream_t st = reinterpret_cast<hipStream_t>(d.stream);
    FwdBufs f;
    layout_fwd(d, s, d.ws, f);
    WBufs w;
    layout_w(s, d.wws, w);
    BwdBufs b;
    layout_bwd(d, s, f, bws, b);
    const int N = s.N, mode = s.mode, lowp = s.lowp ? 1 : 0;
    const long long ldcat = s.seg_off[s.nconv + 1];
    // ---- operand copies the backward consumes (transposes): one launch
    {
        Packer pk(st);
        for (int l = 0; l < s.nconv; ++l) {
            const int Fin = s.Fin[l], H1 = s.H1[l], H1p = s.H1p[l], H2 = s.H2[l];
            pk.add(w.W2T[l], up(H2, 32), lowp, d.W2[l], 1, H1, H1, H2);                          // W2^T: [H1, H2]
            if (l > 0) {                                                                        // [Fin, 2 H1p] = [(Wa - Wb)^T | Wb^T]
                const long long kp = up(2 * H1p, s.ku), ldw = 2LL * Fin;
                pk.add(w.WpqT[l], kp, lowp, d.W1[l], 1, ldw, Fin, H1, d.W1[l] + Fin);
                pk.add(reinterpret_cast<unsigned char*>(w.WpqT[l]) + (long long)H1p * s.es, kp, lowp, d.W1[l] + Fin, 1, ldw, Fin, H1);
            }
        }
        long long ktot0 = 0;
        for (int i = 0; i <= s.nconv; ++i) ktot0 += s.seg_w[i];
        for (int t = 1; t < s.npost; ++t) pk.add(w.postT[t], up(s.P[t], s.ku), lowp, d.Wp[t], 1, s.P[t - 1], s.P[t - 1], s.P[t]);
        {
            long long off = s.seg_w[0];
            for (int i = 1; i <= s.nconv; ++i) {     // rows of segment i at r0 = seg_off[i] - seg_off[1]: W[:, off : off + w]^T
                pk.add(reinterpret_cast<unsigned char*>(w.catT) + (long long)(s.seg_off[i] - s.seg_off[1]) * up(s.P[0], s.ku) * s.es,
                       up(s.P[0], s.ku), lowp, d.Wp[0] + off, 1, ktot0, s.seg_w[i], s.P[0]);
                off += s.seg_w[i];
            }
        }
        pk.flush();
        GN_TRY(pk.err);
    }
    // ---- pooling backward, gated by the last post layer's relu
    const int last = s.npost - 1;
    void* dZ = b.dZ[0];
    int zsel = 0;
    {
        Timed tm(st, "segment_pool_bwd");
        if (s.Pr[last] != s.P[last])
            GN_TRY(hipMemset2DAsync(reinterpret_cast<unsigned char*>(dZ) + (long long)s.P[last] * s.es, (size_t)s.Pr[last] * s.es, 0,
                                    (size_t)(s.Pr[last] - s.P[last]) * s.es, (size_t)N, st));
        GN_TRY(launch_pool_bwd(gout, s.P[last], d.ptr, d.batch, N, d.pool_codes, s.npool, f.amin, f.amax,
                               reinterpret_cast<const float*>(f.y[last]), s.Pr[last], dZ, s.Pr[last], lowp, st));
    }
    Packer unpack(st);          // gradients that need their pad columns dropped / a difference formed: one launch at the end
    float* dwtmp = b.dWtmp;     // (every weight gradient has its own slice of the scratch)
    float* dbtmp = b.dbtmp;
    // ---- post-processing MLP, last layer first
    for (int t = last; t >= 0; --t) {
        const int Pt = s.P[t];
        Segs x;
        std::memset(&x, 0, sizeof(x));
        int ktot = 0;
        bool padded = false;
        if (t == 0) {
            x.nseg = s.nconv + 1;
            for (int i = 0; i <= s.nconv; ++i) {
                x.p[i] = i == 0 ? f.x0 : f.out[i - 1];
                x.ld[i] = i == 0 ? s.ld0 : s.H2[i - 1];
                x.width[i] = s.kw(s.seg_w[i]);
                ktot += x.width[i];
                padded = padded || x.width[i] != s.seg_w[i];
            }
        } else {
            x = one_seg(f.y[t - 1], s.Pr[t - 1], s.kw(s.P[t - 1]), s.ku);
            ktot = x.width[0];
            padded = x.width[0] != s.P[t - 1];
        }
        float* dW = padded ? dwtmp : gr.dWp[t];
        if (padded) dwtmp += (long long)Pt * ktot;
        {
            Timed tm(st, "linear_wgrad", ktot, Pt);
            GN_TRY(launch_gemm_tn(mode, dZ, lowp, s.Pr[t], Pt, x, lowp, N, b.slab, b.dbp, dW, gr.dbp[t], 0, st));
        }
        if (padded) {
            long long ktrue = 0, off = 0, offk = 0;
            if (t == 0) for (int i = 0; i <= s.nconv; ++i) ktrue += s.seg_w[i]; else ktrue = s.P[t - 1];
            const int nseg = t == 0 ? s.nconv + 1 : 1;
            for (int i = 0; i < nseg; ++i) {
                const int wi = t == 0 ? s.seg_w[i] : s.P[t - 1];
                unpack.add(gr.dWp[t] + off, ktrue, 0, dW + offk, ktot, 1, Pt, wi);
                off += wi;
                offk += s.kw(wi);
            }
        }
        if (t > 0) {
            void* dZn = b.dZ[zsel ^ 1];
            const int Pp = s.P[t - 1], Ppr = s.Pr[t - 1];
            if (Ppr != Pp)
                GN_TRY(hipMemset2DAsync(reinterpret_cast<unsigned char*>(dZn) + (long long)Pp * s.es, (size_t)Ppr * s.es, 0,
                                        (size_t)(Ppr - Pp) * s.es, (size_t)N, st));
            Timed tm(st, "linear_fwd", s.kw(Pt), Pp);
            GN_TRY(launch_gemm_nt(mode, one_seg(dZ, s.Pr[t], s.kw(Pt), s.ku), lowp, N, w.postT[t], (int)up(Pt, s.ku), (int)up(Pp, 128), Pp,
                                  epi(nullptr, 0, 0, f.y[t - 1], Ppr, lowp), dZn, Ppr, lowp, st));
            dZ = dZn;
            zsel ^= 1;
        } else {
            // gradient w.r.t. the skip-cat input, segment 0 (the raw pulse features) excluded: nobody reads it
            const int ncols = s.seg_off[s.nconv + 1] - s.seg_off[1];
            Timed tm(st, "linear_fwd", s.kw(Pt), ncols);
            GN_TRY(launch_gemm_nt(mode, one_seg(dZ, s.Pr[t], s.kw(Pt), s.ku), lowp, N, w.catT, (int)up(Pt, s.ku), (int)up(ncols, 128), ncols,
                                  epi(), reinterpret_cast<unsigned char*>(b.dXcat) + (long long)s.seg_off[1] * s.es, ldcat, lowp, st));
        }
    }
    // ---- DynEdgeConv layers, last first
    for (int l = s.nconv - 1; l >= 0; --l) {
        const int Fin = s.Fin[l], H1 = s.H1[l], H1p = s.H1p[l], H2 = s.H2[l];
        const Table& t = f.tab[l];
        const EdgeGraph g = t.graph(N);
        const void* g_out = reinterpret_cast<const unsigned char*>(b.dXcat) + (long long)s.seg_off[l + 1] * s.es;
        const void* xin = l == 0 ? f.x0 : f.out[l - 1];
        const long long ldin = l == 0 ? s.ld0 : s.H2[l - 1];
        const int* hubs = nullptr;
        const int* nhubs = nullptr;
        GN_TRY(build_reverse(s, d, t, b, &hubs, &nhubs, st));
        {
            Timed tm(st, "edgeconv_dw2", H1p, H2);
            GN_TRY(launch_edge_dw2(mode, g, f.PQ[l], H1p, H1, H2, g_out, ldcat, f.saved[l], b.slab, b.dbp, st));
        }
        {
            Timed tm(st, "reduce_slabs");
            GN_TRY(launch_edge_dw2_reduce(mode, g, H1p, H1, H2, b.slab, b.dbp, gr.dW2[l], gr.db2[l], st));
        }
        // dpre (the backward's edge-row tensor, read back once by the source gather) without the elements the h-bits mark
        // as zero where the shape allows it (csrc/dpre_compact.hip): same values summed in the same order
        const bool compact = dpre_compact_supported(mode, t.K, H1p, H1, H2) != 0;
        if (compact) {
            Timed tm(st, "dpre_plan");
            GN_TRY(launch_dpre_plan_saved(N, t.K, H1p, H1, H2, f.saved[l], b.plan, st));
        }
        {
            Timed tm(st, "edgeconv_bwd", H1p, H2);
            if (compact)
                GN_TRY(launch_edge_bwd_cp(g, f.PQ[l], H1p, H1, H2, g_out, ldcat, f.saved[l], w.W2T[l], (int)up(H2, 32), b.plan, b.dpre,
                                          t.cnt ? b.dpre_ovf : nullptr, b.dPQ, 2 * H1p, st));
            else
                GN_TRY(launch_edge_bwd(mode, g, f.PQ[l], H1p, H2, g_out, ldcat, f.saved[l], w.W2T[l], (int)up(H2, 32), b.dpre, b.dPQ, 2 * H1p, st));
        }
        {
            Timed tm(st, "edgeconv_dq_gather");
            void* dQ = reinterpret_cast<unsigned char*>(b.dPQ) + (long long)H1p * s.es;
            if (compact)
                GN_TRY(launch_dq_gather_cp_saved(N, t.K, H1p, H1, H2, f.saved[l], b.plan, b.dpre, t.cnt ? b.dpre_ovf : nullptr, b.rev_ptr,
                                                 b.rev_rows, hubs, nhubs, dQ, 2 * H1p, st));
            else
                GN_TRY(launch_dq_gather(mode, b.dpre, H1p, b.rev_ptr, b.rev_rows, hubs, nhubs, N, dQ, 2 * H1p, st));
        }
        const int wk = s.kw(Fin);
        {
            Timed tm(st, "linear_wgrad", wk, 2 * H1p);
            GN_TRY(launch_gemm_tn(mode, b.dPQ, lowp, 2 * H1p, 2 * H1p, one_seg(xin, ldin, wk, s.ku), lowp, N, b.slab, b.dbp, dwtmp, dbtmp, 0, st));
        }
        // dW1 = [dWp | dWq - dWp] (W1 = [Wa | Wb], P = (Wa - Wb) x + b1, Q = Wb x), db1 = dbpq[:H1]
        unpack.add(gr.dW1[l], 2LL * Fin, 0, dwtmp, wk, 1, H1, Fin);
        unpack.add(gr.dW1[l] + Fin, 2LL * Fin, 0, dwtmp + (long long)H1p * wk, wk, 1, H1, Fin, dwtmp);
        unpack.add(gr.db1[l], H1, 0, dbtmp, H1, 1, 1, H1);
        dwtmp += (long long)2 * H1p * wk;
        dbtmp += 2 * H1p;
        if (l > 0) {
            // d_in += [dP | dQ] . [(Wa - Wb) | Wb]: one K = 2 H1p contraction accumulating into the skip-cat gradient
            Timed tm(st, "linear_fwd", 2 * H1p, Fin);
            GN_TRY(launch_gemm_nt(mode, one_seg(b.dPQ, 2 * H1p, 2 * H1p, s.ku), lowp, N, w.WpqT[l], (int)up(2 * H1p, s.ku), (int)up(Fin, 128), Fin,
                                  epi(nullptr, 0, 1), reinterpret_cast<unsigned char*>(b.dXcat) + (long long)s.seg_off[l] * s.es, ldcat, lowp, st));
        }
    }
    unpack.flush();
    GN_TRY(unpack.err);
    return hipSuccess;
}

}  // namespace gn

// ====================================================================================== C ABI
namespace {
thread_local char s_err[512] = "";
}
extern "C" {

const char* gn_step_last_error(void) { return s_err; }

static int step_fail(hipError_t e, const char* where) {
    if (e == hipSuccess) return 0;
    std::snprintf(s_err, sizeof(s_err), "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
    return (int)e;
}
static int step_bad(const char* where, const char* what) {
    std::snprintf(s_err, sizeof(s_err), "%s: %s", where, what);
    return (int)hipErrorInvalidValue;
}

int64_t gn_dynedge_wws_bytes(const GnDynEdgeDesc* d) {
    gn::Shapes s; const char* why;
    if (!d || !gn::make_shapes(*d, s, &why)) return -1;
    gn::WBufs w;
    gn::layout_w(s, nullptr, w);
    return w.total;
}
int64_t gn_dynedge_ws_bytes(const GnDynEdgeDesc* d) {
    gn::Shapes s; const char* why;
    if (!d || !gn::make_shapes(*d, s, &why)) return -1;
    gn::FwdBufs f;
    gn::layout_fwd(*d, s, nullptr, f);
    return f.total;
}
int64_t gn_dynedge_bwd_ws_bytes(const GnDynEdgeDesc* d) {
    gn::Shapes s; const char* why;
    if (!d || !gn::make_shapes(*d, s, &why)) return -1;
    gn::FwdBufs f;
    gn::layout_fwd(*d, s, nullptr, f);
    gn::BwdBufs b;
    gn::layout_bwd(*d, s, f, nullptr, b);
    return b.total;
}
static int check_desc(const GnDynEdgeDesc* d, gn::Shapes& s, const char* where) {
    const char* why = nullptr;
    if (!d) return step_bad(where, "null descriptor");
    if (!gn::make_shapes(*d, s, &why)) return step_bad(where, why);
    if (!d->x || !d->ptr || !d->batch || !d->n_pulses || !d->ws || !d->wws) return step_bad(where, "x / ptr / batch / n_pulses / ws / wws");
    if ((reinterpret_cast<uintptr_t>(d->ws) & 255) || (reinterpret_cast<uintptr_t>(d->wws) & 255)) return step_bad(where, "workspaces must be 256-byte aligned");
    if (d->ws_bytes < gn_dynedge_ws_bytes(d) || d->wws_bytes < gn_dynedge_wws_bytes(d)) return step_bad(where, "workspace too small (gn_dynedge_ws_bytes / gn_dynedge_wws_bytes)");
    if (d->nbr0 && (d->K0 < 1 || d->K0 > 32)) return step_bad(where, "caller-built layer-1 table: 1 <= K0 <= 32");
    if (!d->nbr0 && (d->n_graph_cols < 1 || d->n_graph_cols > 8)) return step_bad(where, "1..8 layer-1 graph columns");
    for (int l = 0; l < d->nconv; ++l) if (!d->W1[l] || !d->b1[l] || !d->W2[l] || !d->b2[l]) return step_bad(where, "conv parameters");
    for (int t = 0; t < d->npost; ++t) if (!d->Wp[t] || !d->bp[t]) return step_bad(where, "post-MLP parameters");
    for (int c = 0; c < d->npool; ++c) if (d->pool_codes[c] < 0 || d->pool_codes[c] > 3) return step_bad(where, "pool codes 0..3");
    return 0;
}
int gn_dynedge_fwd(const GnDynEdgeDesc* d, float* global_vars, float* pooled) {
    gn::Shapes s;
    if (int rc = check_desc(d, s, "gn_dynedge_fwd")) return rc;
    if (!global_vars || !pooled) return step_bad("gn_dynedge_fwd", "outputs");
    return step_fail(gn::dynedge_fwd(*d, s, global_vars, pooled), "gn_dynedge_fwd");
}
int gn_dynedge_bwd(const GnDynEdgeDesc* d, const float* grad_pooled, void* bws, int64_t bws_bytes, const GnDynEdgeGrads* grads) {
    gn::Shapes s;
    if (int rc = check_desc(d, s, "gn_dynedge_bwd")) return rc;
    if (!grad_pooled || !bws || !grads || (reinterpret_cast<uintptr_t>(bws) & 255)) return step_bad("gn_dynedge_bwd", "grad_pooled / bws (256-byte aligned) / grads");
    if (bws_bytes < gn_dynedge_bwd_ws_bytes(d)) return step_bad("gn_dynedge_bwd", "backward workspace too small (gn_dynedge_bwd_ws_bytes)");
    for (int l = 0; l < d->nconv; ++l) if (!grads->dW1[l] || !grads->db1[l] || !grads->dW2[l] || !grads->db2[l]) return step_bad("gn_dynedge_bwd", "conv gradient outputs");
    for (int t = 0; t < d->npost; ++t) if (!grads->dWp[t] || !grads->dbp[t]) return step_bad("gn_dynedge_bwd", "post-MLP gradient outputs");
    return step_fail(gn::dynedge_bwd(*d, s, grad_pooled, bws, *grads), "gn_dynedge_bwd");
}

// per-op HIP events inside the two entries above (bench.py): enable, run steps, read "name launches total_ms" lines
void gn_step_timers_enable(int32_t on) {
    gn::g_timers_on = on != 0;
    if (!on) {
        for (auto& t : gn::g_timers) { (void)hipEventDestroy(t.a); (void)hipEventDestroy(t.b); }
        gn::g_timers.clear();
    }
}
int64_t gn_step_timers_read(char* buf, int64_t cap) {
    // synchronises the device; returns the bytes needed (incl. the terminator); writes at most cap
    (void)hipDeviceSynchronize();
    std::vector<std::string> names;
    std::vector<double> ms;
    std::vector<long long> cnt;
    for (auto& t : gn::g_timers) {
        float v = 0.0f;
        if (hipEventElapsedTime(&v, t.a, t.b) != hipSuccess) continue;
        size_t i = 0;
        for (; i < names.size(); ++i) if (names[i] == t.name) break;
        if (i == names.size()) { names.push_back(t.name); ms.push_back(0.0); cnt.push_back(0); }
        ms[i] += v; cnt[i] += 1;
    }
    std::string out;
    char line[160];
    for (size_t i = 0; i < names.size(); ++i) {
        std::snprintf(line, sizeof(line), "%s %lld %.6f\n", names[i].c_str(), cnt[i], ms[i]);
        out += line;
    }
    if (buf && cap > 0) {
        const size_t n = out.size() < (size_t)cap - 1 ? out.size() : (size_t)cap - 1;
        std::memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int64_t)out.size() + 1;
}

}  // extern "C"
