// graphnet_amd/csrc/cabi.hip — extern "C" surface declared in include/graphnet_amd.h.
// Plain pointers and sizes only; argument validation lives here so that a bad shape is an
// error code, never a faulting kernel.
#include "../../include/graphnet_amd.h"
#include "launchers.hpp"
#include <cstdio>
#include <cstring>

namespace {
thread_local char g_err[512] = "";
int fail(hipError_t e, const char* where) {
    if (e == hipSuccess) return 0;
    std::snprintf(g_err, sizeof(g_err), "%s: %s (%d)", where, hipGetErrorString(e), (int)e);
    return (int)e;
}
int bad(const char* where, const char* what) {
    std::snprintf(g_err, sizeof(g_err), "%s: %s", where, what);
    return (int)hipErrorInvalidValue;
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

bool make_segs(gn::Segs& s, int nseg, const void* const* p, const int64_t* ld, const int32_t* width,
               const int32_t* kpad) {
    if (nseg < 1 || nseg > gn::MAXSEG) return false;
    std::memset(&s, 0, sizeof(s));
    s.nseg = nseg;
    for (int i = 0; i < nseg; ++i) {
        if (!p[i] || (reinterpret_cast<uintptr_t>(p[i]) & 15)) return false;
        s.p[i] = p[i]; s.ld[i] = ld[i]; s.width[i] = width[i];
        s.kpad[i] = kpad ? kpad[i] : (width[i] + gn::BK - 1) / gn::BK * gn::BK;
    }
    return true;
}
gn::EdgeGraph make_graph(const int32_t* nbr, const int32_t* oc, const int32_t* os, const int32_t* cnt, int N, int K) {
    gn::EdgeGraph g;
    g.nbr = nbr; g.ovf_centre = oc; g.ovf_src = os; g.ovf_cnt = cnt; g.N = N; g.K = K;
    return g;
}
}  // namespace

extern "C" {

const char* gn_last_error(void) { return g_err; }
int gn_abi_version(void) { return GN_ABI_VERSION; }

int gn_knn_plan(const int32_t* ptr, int32_t B, int32_t* tile_ptr, void* stream) {
    if (B < 0 || !ptr || !tile_ptr) return bad("gn_knn_plan", "need ptr[B+1] and tile_ptr[B+1]");
    return fail(gn::launch_knn_plan(ptr, B, tile_ptr, S(stream)), "gn_knn_plan");
}
int gn_knn_graph(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D, const int32_t* ptr,
                 const int32_t* tile_ptr, int32_t B, int32_t N, int32_t k, int32_t strict, int32_t* nbr, int32_t* ovf,
                 void* stream) {
    if (N < 0 || B < 0 || k < 1 || k > 32 || D < 1 || D > 8 || !cols_host) return bad("gn_knn_graph", "need 1<=k<=32, 1<=D<=8");
    if (N > 0 && B > 0 && !tile_ptr) return bad("gn_knn_graph", "needs the tile plan of gn_knn_plan");
    if (!strict && !ovf) return bad("gn_knn_graph", "compat mode needs ovf[N]");
    for (int d = 0; d < D; ++d) if (cols_host[d] < 0 || cols_host[d] >= ldx) return bad("gn_knn_graph", "column out of range");
    return fail(gn::launch_knn(x, ldx, cols_host, D, ptr, tile_ptr, B, N, k, strict, nbr, ovf, nullptr, S(stream)), "gn_knn_graph");
}
int64_t gn_knn_ws_bytes(int32_t B, int32_t N, int32_t D) { return (B < 0 || N < 0 || D < 1 || D > 8) ? -1 : gn::knn_ws_bytes(B, N, D); }
int gn_knn_graph_ws(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D, const int32_t* ptr,
                    const int32_t* tile_ptr, int32_t B, int32_t N, int32_t k, int32_t strict, int32_t* nbr, int32_t* ovf,
                    void* ws, void* stream) {
    if (N < 0 || B < 0 || k < 1 || k > 32 || D < 1 || D > 8 || !cols_host) return bad("gn_knn_graph_ws", "need 1<=k<=32, 1<=D<=8");
    if (N > 0 && B > 0 && !tile_ptr) return bad("gn_knn_graph_ws", "needs the tile plan of gn_knn_plan");
    if (!strict && !ovf) return bad("gn_knn_graph_ws", "compat mode needs ovf[N]");
    for (int d = 0; d < D; ++d) if (cols_host[d] < 0 || cols_host[d] >= ldx) return bad("gn_knn_graph_ws", "column out of range");
    return fail(gn::launch_knn(x, ldx, cols_host, D, ptr, tile_ptr, B, N, k, strict, nbr, ovf, ws, S(stream)), "gn_knn_graph_ws");
}
int gn_minkowski_knn_graph(const float* x, int64_t ldx, const int32_t* space_cols_host, int32_t DS, int32_t time_col,
                           float c, float time_like_weight, const int32_t* ptr, const int32_t* tile_ptr,
                           int32_t B, int32_t N, int32_t k, int32_t* nbr, void* stream) {
    const char* me = "gn_minkowski_knn_graph";
    if (N < 0 || B < 0 || k < 1 || k > 32 || DS < 1 || DS > 7) return bad(me, "need 1<=k<=32, 1<=DS<=7");
    if (time_col < 0 || time_col >= ldx) return bad(me, "time column out of range");
    if (!space_cols_host) return bad(me, "need space_cols_host[DS]");
    for (int d = 0; d < DS; ++d) if (space_cols_host[d] < 0 || space_cols_host[d] >= ldx) return bad(me, "space column out of range");
    if (N > 0 && B > 0 && !tile_ptr) return bad(me, "needs the tile plan of gn_knn_plan");
    if (N > 0 && B > 0 && (!x || !ptr || !nbr)) return bad(me, "need x, ptr[B+1] and nbr[N, k]");
    return fail(gn::launch_minkowski_knn(x, ldx, space_cols_host, DS, time_col, c, time_like_weight, ptr, tile_ptr, B, N, k,
                                         nbr, S(stream)), me);
}
int64_t gn_radius_work_ints(int32_t B, int32_t N) { return (B < 0 || N < 0) ? -1 : gn::radius_work_ints(B, N); }
int gn_radius_graph(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D, float r, const int32_t* ptr,
                    const int32_t* tile_ptr, int32_t B, int32_t N, int32_t cap, int32_t* nbr, int32_t* deg, int32_t* work,
                    void* stream) {
    const char* me = "gn_radius_graph";
    if (N < 0 || B < 0 || cap < 1 || cap > 32 || D < 1 || D > 8) return bad(me, "need 1<=cap<=32, 1<=D<=8");
    if (!(r > 0.0f) || !(r <= 3.4028234e38f)) return bad(me, "need a finite radius > 0");
    if (!cols_host) return bad(me, "need cols_host[D]");
    for (int d = 0; d < D; ++d) if (cols_host[d] < 0 || cols_host[d] >= ldx) return bad(me, "column out of range");
    if (!tile_ptr) return bad(me, "needs the tile plan of gn_knn_plan");
    if (N > 0 && B > 0 && (!x || !ptr || !nbr || !deg || !work))
        return bad(me, "need x, ptr[B+1], nbr[N, cap], deg[N] and work[gn_radius_work_ints(B, N)]");
    return fail(gn::launch_radius_graph(x, ldx, cols_host, D, r, ptr, tile_ptr, B, N, cap, nbr, deg, work, S(stream)), me);
}

int64_t gn_percentile_work_ints(int32_t B, int32_t N) { return (B < 0 || N < 0) ? -1 : gn::percentile_work_ints(B, N); }
int32_t gn_percentile_lds_max(void) { return gn::percentile_lds_max(); }
// NS: the header's S (S() is the stream cast in this file)
int gn_percentile_clusters(const float* x, int64_t ldx, int32_t N, const int32_t* ptr, int32_t B,
                           const int32_t* cluster_cols_host, int32_t C, const int32_t* summ_cols_host, int32_t NS,
                           const double* q_host, int32_t P, int32_t add_counts, float* out, int64_t ldo, int32_t* out_ptr,
                           int32_t* work, void* stream) {
    const char* me = "gn_percentile_clusters";
    if (N < 0 || B < 0 || N > (1 << 28)) return bad(me, "need B >= 0 and 0 <= N <= 2^28");
    if (C < 1 || C > 8 || NS < 1 || NS > 32 || P < 1 || P > 16) return bad(me, "need 1<=C<=8, 1<=S<=32, 1<=P<=16");
    if (!cluster_cols_host || !summ_cols_host || !q_host) return bad(me, "need cluster_cols_host[C], summ_cols_host[S] and q_host[P]");
    for (int p = 0; p < P; ++p) if (!(q_host[p] >= 0.0 && q_host[p] <= 1.0)) return bad(me, "need 0 <= q <= 1");
    for (int i = 0; i < C + NS; ++i) {
        const int ci = i < C ? cluster_cols_host[i] : summ_cols_host[i - C];
        if (ci < 0 || ci >= ldx) return bad(me, "column out of range");
        for (int j = 0; j < i; ++j)
            if (ci == (j < C ? cluster_cols_host[j] : summ_cols_host[j - C])) return bad(me, "columns must be distinct");
    }
    if (ldo < (int64_t)C + (int64_t)NS * P + (add_counts ? 1 : 0)) return bad(me, "need ldo >= C + S*P + add_counts");
    if (B > 0 && (!ptr || !out_ptr)) return bad(me, "need ptr[B+1] and out_ptr[B+1]");
    if (N > 0 && B > 0 && (!x || !out || !work)) return bad(me, "need x, out[N, ldo] and work[gn_percentile_work_ints(B, N)]");
    return fail(gn::launch_percentile_clusters(x, ldx, N, ptr, B, cluster_cols_host, C, summ_cols_host, NS, q_host, P,
                                               add_counts ? 1 : 0, out, ldo, out_ptr, work, S(stream)), me);
}

int64_t gn_dom_time_series_work_ints(int32_t B, int32_t N) { return (B < 0 || N < 0) ? -1 : gn::dom_time_series_work_ints(B, N); }
int gn_dom_time_series(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* ptr, int32_t B,
                       const int32_t* id_cols_host, int32_t C, int32_t time_col, int32_t charge_col, float* out, int64_t ldo,
                       int32_t* series_ptr, int32_t* dom_ptr, int32_t* work, void* stream) {
    const char* me = "gn_dom_time_series";
    if (N < 0 || B < 0 || N > (1 << 28)) return bad(me, "need B >= 0 and 0 <= N <= 2^28");
    if (F < 1 || F > ldx) return bad(me, "need 1 <= F <= ldx");
    if (C < 1 || C > 8 || !id_cols_host) return bad(me, "need id_cols_host[C], 1<=C<=8");
    if (time_col < 0 || time_col >= F || charge_col < -1 || charge_col >= F || charge_col == time_col)
        return bad(me, "time / charge column out of range (charge_col = -1: none)");
    for (int i = 0; i < C; ++i) {
        const int ci = id_cols_host[i];
        if (ci < 0 || ci >= F) return bad(me, "column out of range");
        if (ci == time_col || ci == charge_col) return bad(me, "columns must be distinct");
        for (int j = 0; j < i; ++j) if (ci == id_cols_host[j]) return bad(me, "columns must be distinct");
    }
    if (ldo < (int64_t)F + (charge_col < 0 ? 1 : 0) + 1) return bad(me, "need ldo >= F + (charge_col < 0) + 1");
    if (!series_ptr) return bad(me, "need series_ptr[N+1]");
    if (B > 0 && (!ptr || !dom_ptr)) return bad(me, "need ptr[B+1] and dom_ptr[B+1]");
    if (N > 0 && B > 0 && (!x || !out || !work)) return bad(me, "need x, out[N, ldo] and work[gn_dom_time_series_work_ints(B, N)]");
    return fail(gn::launch_dom_time_series(x, ldx, F, N, ptr, B, id_cols_host, C, time_col, charge_col, out, ldo, series_ptr,
                                           dom_ptr, work, S(stream)), me);
}

int gn_icemix_nodes(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* ptr, int32_t B, int32_t max_pulses,
                    int32_t hlc_col, int32_t z_col, const double* table, int32_t T, uint32_t seed, const uint32_t* event_ids,
                    int32_t key_bits, float* out, int64_t ldo, int32_t* out_ptr, int32_t* ids, void* stream) {
    const char* me = "gn_icemix_nodes";
    if (N < 0 || B < 0 || N > (1 << 28)) return bad(me, "need B >= 0 and 0 <= N <= 2^28");
    if (F < 1 || F > ldx) return bad(me, "need 1 <= F <= ldx");
    if (max_pulses < 1) return bad(me, "need max_pulses >= 1");
    if (key_bits < 1 || key_bits > 32) return bad(me, "need 1 <= key_bits <= 32");
    if (hlc_col < -1 || hlc_col >= F || z_col < -1 || z_col >= F) return bad(me, "hlc / z column out of range (-1: none)");
    if (z_col >= 0 && (T < 2 || T > 1024 || !table)) return bad(me, "ice columns need table[3*T], 2 <= T <= 1024");
    if (ldo < (int64_t)F + (z_col >= 0 ? 2 : 0)) return bad(me, "need ldo >= F + 2*(z_col >= 0)");
    if (B > 0 && (!ptr || !out_ptr)) return bad(me, "need ptr[B+1] and out_ptr[B+1]");
    if (N > 0 && B > 0 && (!x || !out || !ids)) return bad(me, "need x, out[M, ldo] and ids[M]");
    return fail(gn::launch_icemix_nodes(x, ldx, F, N, ptr, B, max_pulses, hlc_col, z_col, table, T, seed, event_ids, key_bits,
                                        out, ldo, out_ptr, ids, S(stream)), me);
}

int32_t gn_gru_supported(int32_t I, int32_t H) { return gn::gru_supported(I, H); }
int64_t gn_gru_saved_floats(int32_t T, int32_t H) { return (T < 0 || H < 1) ? -1 : gn::gru_saved_floats(T, H); }
int64_t gn_gru_bwd_work_floats(int32_t T, int32_t I, int32_t H) {
    return (T < 0 || !gn::gru_supported(I, H)) ? -1 : gn::gru_bwd_work_floats(T, I, H);
}
int gn_gru_series_fwd(const float* xs, int64_t ldx, int32_t T, int32_t I, const int32_t* series_ptr, int32_t M, int32_t H,
                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out, float* saved,
                      void* stream) {
    const char* me = "gn_gru_series_fwd";
    if (!gn::gru_supported(I, H)) return bad(me, "outside the envelope: need 1<=I<=32, 4<=H<=64, H%4==0 (gn_gru_supported)");
    if (T < 0 || M < 0 || M > T || ldx < I) return bad(me, "need 0 <= M <= T (no empty series) and ldx >= I");
    if (!w_ih || !w_hh || !b_ih || !b_hh) return bad(me, "need weight_ih[3H, I], weight_hh[3H, H], bias_ih[3H], bias_hh[3H]");
    if (M > 0 && (!xs || !series_ptr || !out)) return bad(me, "need xs[T, ldx], series_ptr[M+1] and out[M, H]");
    if (reinterpret_cast<uintptr_t>(saved) & 15) return bad(me, "saved must be 16-byte aligned");
    return fail(gn::launch_gru_series_fwd(xs, ldx, T, I, series_ptr, M, H, w_ih, w_hh, b_ih, b_hh, out, saved, S(stream)), me);
}
int gn_gru_series_bwd(const float* dout, const float* saved, const float* xs, int64_t ldx, int32_t T, int32_t I,
                      const int32_t* series_ptr, int32_t M, int32_t H, const float* w_hh, float* dw_ih, float* db_ih,
                      float* dw_hh, float* db_hh, float* work, void* stream) {
    const char* me = "gn_gru_series_bwd";
    if (!gn::gru_supported(I, H)) return bad(me, "outside the envelope: need 1<=I<=32, 4<=H<=64, H%4==0 (gn_gru_supported)");
    if (T < 0 || M < 0 || M > T || ldx < I) return bad(me, "need 0 <= M <= T (no empty series) and ldx >= I");
    if (!w_hh || !dw_ih || !db_ih || !dw_hh || !db_hh) return bad(me, "need weight_hh and the four gradient buffers");
    if (M > 0 && (!dout || !saved || !xs || !series_ptr || !work))
        return bad(me, "need dout[M, H], saved, xs[T, ldx], series_ptr[M+1] and work[gn_gru_bwd_work_floats(T, I, H)]");
    if ((reinterpret_cast<uintptr_t>(saved) & 15) || (reinterpret_cast<uintptr_t>(work) & 15))
        return bad(me, "saved and work must be 16-byte aligned");
    return fail(gn::launch_gru_series_bwd(dout, saved, xs, ldx, T, I, series_ptr, M, H, w_hh, dw_ih, db_ih, dw_hh, db_hh, work,
                                          S(stream)), me);
}
int gn_dom_series_summary(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* series_ptr, int32_t M,
                          int32_t charge_col, float* out, int64_t ldo, void* stream) {
    const char* me = "gn_dom_series_summary";
    if (N < 0 || M < 0 || M > N) return bad(me, "need 0 <= M <= N");
    if (F < 1 || F > ldx || ldo < F) return bad(me, "need 1 <= F <= ldx and ldo >= F");
    if (charge_col < 0 || charge_col >= F) return bad(me, "charge column out of range");
    if (M > 0 && (!x || !series_ptr || !out)) return bad(me, "need x[N, ldx], series_ptr[M+1] and out[M, ldo]");
    return fail(gn::launch_dom_series_summary(x, ldx, F, N, series_ptr, M, charge_col, out, ldo, S(stream)), me);
}

int64_t gn_scan_tmp_ints(int64_t n) { return (n + 2047) / 2048 + 1; }
int gn_scan_i32(const int32_t* in, int32_t* out, int32_t n, int32_t* tmp, int32_t* total, void* stream) {
    if (n < 0) return bad("gn_scan_i32", "n < 0");
    return fail(gn::launch_scan(in, out, n, tmp, total, S(stream)), "gn_scan_i32");
}
int gn_ovf_compact(const int32_t* ovf, int32_t N, int32_t* work_N, int32_t* tmp, int32_t* ovf_centre,
                   int32_t* ovf_src, int32_t* ovf_cnt, void* stream) {
    return fail(gn::launch_ovf_compact(ovf, N, work_N, tmp, ovf_centre, ovf_src, ovf_cnt, S(stream)), "gn_ovf_compact");
}
int32_t gn_edge_slots(int32_t K) { return gn::edge_slots(K); }
int gn_rev_build(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf_src, const int32_t* ovf_cnt,
                 int32_t* rev_ptr, int32_t* cursor, int32_t* tmp, int32_t* rev_rows, void* stream) {
    if (K < 1 || K > 32) return bad("gn_rev_build", "need 1<=K<=32");
    return fail(gn::launch_rev_build(nbr, N, K, gn::edge_slots(K), ovf_src, ovf_cnt, rev_ptr, cursor, tmp, rev_rows,
                                     S(stream)), "gn_rev_build");
}
int32_t gn_rev_event_slices(int32_t B) { return gn::rev_event_slices(B); }
int gn_rev_build_events(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf, const int32_t* ovf_pos,
                        const int32_t* ptr, int32_t B, int32_t* rev_ptr, int32_t* rev_rows, int32_t* ev, int32_t* scratch,
                        int32_t* hubs, int32_t* nhubs, int32_t* tmp, void* stream) {
    if (K < 1 || K > 32) return bad("gn_rev_build_events", "need 1<=K<=32");
    hipError_t r = gn::launch_rev_build_events(nbr, N, K, gn::edge_slots(K), ovf, ovf_pos, ptr, B, rev_ptr, rev_rows, ev,
                                               scratch, hubs, nhubs, tmp, nullptr, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_rev_build_events", "row ids must fit 31 bits");
    return fail(r, "gn_rev_build_events");
}
int64_t gn_rev_pairs_ints(int32_t B, int32_t N, int32_t K) { return (B < 0 || N < 0 || K < 1 || K > 32) ? -1 : gn::rev_pairs_ints(B, N, K); }
int gn_rev_build_events_ws(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf, const int32_t* ovf_pos,
                           const int32_t* ptr, int32_t B, int32_t* rev_ptr, int32_t* rev_rows, int32_t* ev, int32_t* scratch,
                           int32_t* hubs, int32_t* nhubs, int32_t* tmp, int32_t* pairs, void* stream) {
    if (K < 1 || K > 32) return bad("gn_rev_build_events_ws", "need 1<=K<=32");
    hipError_t r = gn::launch_rev_build_events(nbr, N, K, gn::edge_slots(K), ovf, ovf_pos, ptr, B, rev_ptr, rev_rows, ev,
                                               scratch, hubs, nhubs, tmp, pairs, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_rev_build_events_ws", "row ids must fit 31 bits");
    return fail(r, "gn_rev_build_events_ws");
}
int gn_table_degree(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, int32_t* deg, void* stream) {
    return fail(gn::launch_table_degree(nbr, ovf, N, K, deg, S(stream)), "gn_table_degree");
}
int gn_table_to_edge_index(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, const int32_t* off, int64_t E,
                           int64_t* edge_index, void* stream) {
    return fail(gn::launch_table_to_edges(nbr, ovf, N, K, off, E, reinterpret_cast<long long*>(edge_index), S(stream)),
                "gn_table_to_edge_index");
}
int gn_edge_index_to_table(const int64_t* edge_index, int64_t E, int32_t N, int32_t K, int32_t* first_N, int32_t* nbr,
                           int32_t* ovf, int32_t* err, void* stream) {
    return fail(gn::launch_edges_to_table(reinterpret_cast<const long long*>(edge_index), E, N, K, first_N, nbr, ovf,
                                          err, S(stream)), "gn_edge_index_to_table");
}
int gn_ptr_to_batch(const int32_t* ptr, int32_t B, int32_t* batch, void* stream) {
    return fail(gn::launch_ptr_to_batch(ptr, B, batch, S(stream)), "gn_ptr_to_batch");
}
int gn_standardize(float* x, int64_t ldx, int32_t N, int32_t F, const int32_t* nops_host, const int32_t* op_host,
                   const float* const_host, void* stream) {
    if (!nops_host || !op_host || !const_host || ldx < F) return bad("gn_standardize", "programs / pitch");
    hipError_t r = gn::launch_standardize(x, ldx, N, F, nops_host, op_host, const_host, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_standardize", "need 1 <= F <= 32, <= 3 steps per column, op codes 0..4");
    return fail(r, "gn_standardize");
}
int gn_graph_globals(const float* x, int64_t ldx, int32_t F, const int32_t* ptr, int32_t B, const int32_t* nbr,
                     const int32_t* ovf, int32_t K, const int32_t* n_pulses, float* out, void* stream) {
    if (F < 4 || F > 32 || ldx < F) return bad("gn_graph_globals", "need 4 <= F <= 32 (columns 0-3 = x,y,z,t)");
    return fail(gn::launch_globals(x, ldx, F, ptr, B, nbr, ovf, K, n_pulses, out, S(stream)), "gn_graph_globals");
}
int64_t gn_event_scratch_bytes(int32_t B, int32_t N, int32_t C) {
    const long long a = gn::globals_scratch_bytes(B, N), b = gn::pool_scratch_bytes(B, N, C);
    return a > b ? a : b;
}
int gn_graph_globals_ws(const float* x, int64_t ldx, int32_t F, const int32_t* ptr, int32_t B, int32_t N, const int32_t* nbr,
                        const int32_t* ovf, int32_t K, const int32_t* n_pulses, float* out, void* scratch, void* stream) {
    if (F < 4 || F > 32 || ldx < F) return bad("gn_graph_globals", "need 4 <= F <= 32 (columns 0-3 = x,y,z,t)");
    return fail(gn::launch_globals(x, ldx, F, ptr, B, nbr, ovf, K, n_pulses, out, S(stream), scratch, N), "gn_graph_globals");
}
int gn_concat_globals(const float* x, int64_t ldx, int32_t F, const float* gv, int32_t G, const int32_t* batch,
                      int32_t N, void* x0, int32_t ld0, int32_t out_lowp, void* stream) {
    if (ld0 < F + G) return bad("gn_concat_globals", "ld0 < F+G");
    return fail(gn::launch_concat_globals(x, ldx, F, gv, G, batch, N, x0, ld0, out_lowp, S(stream)), "gn_concat_globals");
}

int gn_linear_fwd(int32_t mode, int32_t nseg, const void* const* a_ptr, int32_t a_lowp, const int64_t* a_ld,
                  const int32_t* a_width, const int32_t* a_kpad, int32_t M, const void* Wp, int32_t Kp, int32_t Npad,
                  int32_t Nreal, const float* bias, const void* gate, int32_t gate_lowp, int64_t ldgate, int32_t relu,
                  int32_t accum, void* C, int64_t ldc, int32_t out_lowp, void* stream) {
    gn::Segs a;
    if (!make_segs(a, nseg, a_ptr, a_ld, a_width, a_kpad)) return bad("gn_linear_fwd", "bad A segments (1..6, 16-byte aligned)");
    if (mode != 0 && mode != 1) return bad("gn_linear_fwd", "mode");
    if ((out_lowp || a_lowp || gate_lowp) && mode == 0) return bad("gn_linear_fwd", "bf16 tensors need bf16 mode");
    if (Npad % 128 || Nreal > Npad || (reinterpret_cast<uintptr_t>(Wp) & 15)) return bad("gn_linear_fwd", "Wp must be [Npad%128==0][Kp], 16-byte aligned");
    gn::Epi e;
    e.bias = bias; e.gate = gate; e.ldgate = ldgate; e.relu = relu; e.accum = accum; e.gate_lowp = gate_lowp;
    hipError_t r = gn::launch_gemm_nt(mode, a, a_lowp, M, Wp, Kp, Npad, Nreal, e, C, ldc, out_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_linear_fwd", "segment widths/pitches must be multiples of 4 (8 for bf16 rows), kpad multiples of 32 summing to Kp");
    return fail(r, "gn_linear_fwd");
}
int32_t gn_linear_wgrad_parts(int32_t mode, int32_t M, int32_t N1, int32_t nseg, const int32_t* x_width) {
    if (nseg < 1 || nseg > gn::MAXSEG || !x_width) return -1;
    return gn::gemm_tn_parts(mode, M, N1, x_width, nseg);
}
int gn_linear_wgrad(int32_t mode, const void* dY, int32_t dy_lowp, int64_t lddy, int32_t N1, int32_t nseg,
                    const void* const* x_ptr, int32_t x_lowp, const int64_t* x_ld, const int32_t* x_width, int32_t M,
                    float* slab, float* db_part, float* dW, float* db, int32_t accum, void* stream) {
    gn::Segs x;
    if (!make_segs(x, nseg, x_ptr, x_ld, x_width, nullptr)) return bad("gn_linear_wgrad", "bad X segments");
    if (reinterpret_cast<uintptr_t>(dY) & 15) return bad("gn_linear_wgrad", "dY must be 16-byte aligned");
    if (db && !db_part) return bad("gn_linear_wgrad", "db needs db_part scratch");
    hipError_t r = gn::launch_gemm_tn(mode, dY, dy_lowp, lddy, N1, x, x_lowp, M, slab, db_part, dW, db, accum, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_linear_wgrad", "widths/pitches/N1 must be multiples of 4 (8 for bf16 rows); bf16 rows need bf16 mode");
    return fail(r, "gn_linear_wgrad");
}
int32_t gn_colsum_blocks(int32_t M) { return gn::colsum_blocks(M); }
int gn_colsum(const float* X, int64_t ld, int32_t M, int32_t C, float* part, float* out, int32_t accum, void* stream) {
    return fail(gn::launch_colsum(X, ld, M, C, part, out, accum, S(stream)), "gn_colsum");
}
int gn_reduce_slabs(const float* slab, int32_t nslab, int64_t count, float* out, int32_t accum, void* stream) {
    return fail(gn::launch_reduce_slabs(slab, nslab, count, out, accum, S(stream)), "gn_reduce_slabs");
}

int64_t gn_edgeconv_saved_bytes(int32_t N, int32_t K, int32_t H1p, int32_t H2) {
    return gn::saved_layout(N, gn::edge_slots(K), H1p, H2).total;
}
void gn_edgeconv_saved_offsets(int32_t N, int32_t K, int32_t H1p, int32_t H2, int64_t* offsets_host) {
    const gn::SavedLayout L = gn::saved_layout(N, gn::edge_slots(K), H1p, H2);
    offsets_host[0] = L.off_words; offsets_host[1] = L.off_maskB; offsets_host[2] = L.off_hbits;
}
int gn_edgeconv_fwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, const void* W2p,
                    const float* b2, int32_t H2, void* out, int64_t ldo, float* coords, const int32_t* coord_cols_host,
                    int32_t ncoord, void* saved, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H2 < 1 || H1 < 1 || H1 > H1p) return bad("gn_edgeconv_fwd", "need 1<=K<=32, H1p%32==0, 1<=H1<=H1p");
    if ((reinterpret_cast<uintptr_t>(PQ) & 15) || (reinterpret_cast<uintptr_t>(W2p) & 15) ||
        (reinterpret_cast<uintptr_t>(saved) & 15)) return bad("gn_edgeconv_fwd", "alignment");
    if (ncoord < 0 || ncoord > 8 || (ncoord > 0 && coords && !coord_cols_host)) return bad("gn_edgeconv_fwd", "0..8 coordinate columns");
    return fail(gn::launch_edge_fwd(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H1, W2p, b2, H2, out,
                                    ldo, coords, coord_cols_host, ncoord, saved, S(stream)), "gn_edgeconv_fwd");
}
int32_t gn_edgeconv_dw2_slabs(int32_t mode, int32_t N, int32_t K, int32_t H1p, int32_t H2) {
    return gn::edge_dw2_slabs(mode, N, K, H1p, H2);
}
void gn_edgeconv_plan(int32_t mode, int32_t K, int64_t N, int32_t H1p, int32_t H1, int32_t H2, int32_t act, int32_t has_ovf,
                      int32_t* plan_host) {
    int out[8];
    gn::edge_plan_query(mode, K, N, H1p, H1, H2, act, has_ovf != 0, out);
    for (int i = 0; i < 8; ++i) plan_host[i] = out[i];
}
int gn_edgeconv_dw2(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                    const void* gout, int64_t ldg, void* saved, float* slab, float* db2_part, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H1 > H1p || (ldg & (mode ? 7 : 3)) || (H2 & 3) || N < 1 ||
        (reinterpret_cast<uintptr_t>(gout) & 15))
        return bad("gn_edgeconv_dw2", "bad shapes");
    return fail(gn::launch_edge_dw2(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H1, H2, gout, ldg,
                                    saved, slab, db2_part, S(stream)), "gn_edgeconv_dw2");
}
int gn_edgeconv_dw2_reduce(int32_t mode, const int32_t* ovf_cnt, int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2,
                           int32_t leaky, const float* slab, const float* db2_part, float* dW2, float* db2, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H1 < 1 || H1 > H1p || N < 1 || !slab || !db2_part || !dW2 || !db2)
        return bad("gn_edgeconv_dw2_reduce", "bad shapes");
    return fail(gn::launch_edge_dw2_reduce(mode, make_graph(nullptr, nullptr, nullptr, ovf_cnt, N, K), H1p, H1, H2, slab, db2_part,
                                           dW2, db2, S(stream), leaky ? 2 : 0), "gn_edgeconv_dw2_reduce");
}
int gn_edgeconv_bwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H2,
                    const void* gout, int64_t ldg, const void* saved, const void* W2Tp, int32_t H2p, void* dpre,
                    void* dP, int64_t ldp, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H2p % 32 || H2p < H2 || (ldg & (mode ? 7 : 3)) || (ldp & (mode ? 7 : 3)) ||
        (reinterpret_cast<uintptr_t>(gout) & 15) || (reinterpret_cast<uintptr_t>(dP) & 15))
        return bad("gn_edgeconv_bwd", "need 1<=K<=32, H1p%32==0, H2p%32==0, gout/dP 16-byte aligned with 16-byte row pitches");
    return fail(gn::launch_edge_bwd(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H2, gout, ldg,
                                    saved, W2Tp, H2p, dpre, dP, ldp, S(stream)), "gn_edgeconv_bwd");
}
// ---- EdgeConvTito (leaky relu edge MLP, max aggregation): fused bf16 kernels
int32_t gn_edgeconv_max_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H2) {
    return gn::edge_max_supported(mode, K, H1p, H2);
}
int32_t gn_edgeconv_max_dw2_slabs(int32_t N, int32_t K, int32_t H1p) { return gn::edge_max_dw2_slabs(N, K, H1p); }
int gn_edgeconv_max_fwd(const int32_t* nbr, int32_t N, int32_t K, const void* PQ, int32_t H1p, const void* W2p,
                        const float* b2, int32_t H2, void* out, int64_t ldo, void* saved, void* stream) {
    if (K < 1 || K > 16 || N < 0 || (reinterpret_cast<uintptr_t>(PQ) & 15) || (reinterpret_cast<uintptr_t>(W2p) & 15) ||
        (reinterpret_cast<uintptr_t>(saved) & 15))
        return bad("gn_edgeconv_max_fwd", "need 1<=K<=16 and 16-byte aligned PQ / W2p / saved");
    hipError_t r = gn::launch_edge_fwd(1, make_graph(nbr, nullptr, nullptr, nullptr, N, K), PQ, H1p, H1p, W2p, b2, H2, out, ldo,
                                       nullptr, nullptr, 0, saved, S(stream), 1);
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_max_fwd", "shape outside the fused envelope (gn_edgeconv_max_supported)");
    return fail(r, "gn_edgeconv_max_fwd");
}
int gn_edgeconv_max_dw2(const int32_t* nbr, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                        const void* gout, int64_t ldg, void* saved, float* slab, float* db2_part, void* stream) {
    if (K < 1 || K > 16 || N < 1 || H1 > H1p || (ldg & 7) || (reinterpret_cast<uintptr_t>(gout) & 15))
        return bad("gn_edgeconv_max_dw2", "bad shapes");
    hipError_t r = gn::launch_edge_dw2(1, make_graph(nbr, nullptr, nullptr, nullptr, N, K), PQ, H1p, H1, H2, gout, ldg, saved,
                                       slab, db2_part, S(stream), 1);
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_max_dw2", "shape outside the fused envelope (gn_edgeconv_max_supported)");
    return fail(r, "gn_edgeconv_max_dw2");
}
int gn_edgeconv_max_bwd(const int32_t* nbr, int32_t N, int32_t K, int32_t H1p, int32_t H2, const void* gout, int64_t ldg,
                        const void* saved, const void* W2Tp, int32_t H2p, void* dpre, void* dP, int64_t ldp, void* stream) {
    if (K < 1 || K > 16 || N < 0 || (ldg & 7) || (ldp & 7) || (reinterpret_cast<uintptr_t>(gout) & 15) ||
        (reinterpret_cast<uintptr_t>(dP) & 15))
        return bad("gn_edgeconv_max_bwd", "need 1<=K<=16, gout / dP 16-byte aligned with 16-byte row pitches");
    hipError_t r = gn::launch_edge_bwd(1, make_graph(nbr, nullptr, nullptr, nullptr, N, K), nullptr, H1p, H2, gout, ldg, saved, W2Tp,
                                       H2p, dpre, dP, ldp, S(stream), 1, H1p);
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_max_bwd", "shape outside the fused envelope (gn_edgeconv_max_supported)");
    return fail(r, "gn_edgeconv_max_bwd");
}

// ---- DynEdgeJINST edge convolution (leaky relu after both layers, add aggregation): arguments as the relu entries
int32_t gn_edgeconv_leaky_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H1, int32_t H2) {
    return gn::edge_leaky_supported(mode, K, H1p, H1, H2);
}
int gn_edgeconv_leaky_fwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, const void* W2p,
                          const float* b2, int32_t H2, void* out, int64_t ldo, float* coords, const int32_t* coord_cols_host,
                          int32_t ncoord, void* saved, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H2 < 1 || H1 < 1 || H1 > H1p) return bad("gn_edgeconv_leaky_fwd", "need 1<=K<=32, H1p%32==0, 1<=H1<=H1p");
    if ((reinterpret_cast<uintptr_t>(PQ) & 15) || (reinterpret_cast<uintptr_t>(W2p) & 15) ||
        (reinterpret_cast<uintptr_t>(saved) & 15)) return bad("gn_edgeconv_leaky_fwd", "alignment");
    if (ncoord < 0 || ncoord > 8 || (ncoord > 0 && coords && !coord_cols_host)) return bad("gn_edgeconv_leaky_fwd", "0..8 coordinate columns");
    return fail(gn::launch_edge_fwd(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H1, W2p, b2, H2, out,
                                    ldo, coords, coord_cols_host, ncoord, saved, S(stream), 2), "gn_edgeconv_leaky_fwd");
}
int gn_edgeconv_leaky_dw2(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                          const void* gout, int64_t ldg, void* saved, float* slab, float* db2_part, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H1 > H1p || (ldg & (mode ? 7 : 3)) || (H2 & 3) || N < 1 ||
        (reinterpret_cast<uintptr_t>(gout) & 15))
        return bad("gn_edgeconv_leaky_dw2", "bad shapes");
    return fail(gn::launch_edge_dw2(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H1, H2, gout, ldg,
                                    saved, slab, db2_part, S(stream), 2), "gn_edgeconv_leaky_dw2");
}
int gn_edgeconv_leaky_bwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                          const void* gout, int64_t ldg, const void* saved, const void* W2Tp, int32_t H2p, void* dpre,
                          void* dP, int64_t ldp, void* stream) {
    if (K < 1 || K > 32 || H1p % 32 || H1 < 1 || H1 > H1p || H2p % 32 || H2p < H2 || (ldg & (mode ? 7 : 3)) ||
        (ldp & (mode ? 7 : 3)) || (reinterpret_cast<uintptr_t>(gout) & 15) || (reinterpret_cast<uintptr_t>(dP) & 15))
        return bad("gn_edgeconv_leaky_bwd", "need 1<=K<=32, H1p%32==0, 1<=H1<=H1p, H2p%32==0, gout/dP 16-byte aligned with 16-byte row pitches");
    return fail(gn::launch_edge_bwd(mode, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H2, gout, ldg,
                                    saved, W2Tp, H2p, dpre, dP, ldp, S(stream), 2, H1), "gn_edgeconv_leaky_bwd");
}

// ---- compact dpre: the backward's edge-row tensor without the elements the stored h-bits mark as zero
int32_t gn_edgeconv_dpre_compact_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H1, int32_t H2) {
    return gn::dpre_compact_supported(mode, K, H1p, H1, H2);
}
int64_t gn_edgeconv_dpre_plan_bytes(int32_t N, int32_t K) { return gn::dpre_plan_layout(N, K, nullptr).total; }
int64_t gn_edgeconv_dpre_compact_bytes(int32_t N, int32_t K, int32_t H1p) { return gn::dpre_compact_bytes(N, K, H1p); }
int gn_edgeconv_dpre_plan(int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2, const void* saved, void* plan, void* stream) {
    if (K < 1 || K > 16 || N < 0 || !saved || !plan || (reinterpret_cast<uintptr_t>(plan) & 255))
        return bad("gn_edgeconv_dpre_plan", "need 1<=K<=16, saved, 256-byte aligned plan workspace");
    hipError_t r = gn::launch_dpre_plan_saved(N, K, H1p, H1, H2, saved, plan, S(stream));
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_dpre_plan", "shape outside the compact envelope (gn_edgeconv_dpre_compact_supported)");
    return fail(r, "gn_edgeconv_dpre_plan");
}
int gn_edgeconv_bwd_compact(const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src, const int32_t* ovf_cnt,
                            int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2, const void* gout, int64_t ldg,
                            const void* saved, const void* W2Tp, int32_t H2p, void* plan, void* dpre_c, void* dpre_ovf, void* dP,
                            int64_t ldp, void* stream) {
    if (K < 1 || K > 16 || (reinterpret_cast<uintptr_t>(gout) & 15) || (reinterpret_cast<uintptr_t>(dP) & 15) ||
        (reinterpret_cast<uintptr_t>(dpre_c) & 15) || !plan || !dpre_c || (ovf_cnt && !dpre_ovf))
        return bad("gn_edgeconv_bwd_compact", "need 1<=K<=16, 16-byte aligned gout / dP / dpre_c, plan, dpre_ovf with an overflow list");
    hipError_t r = gn::launch_edge_bwd_cp(make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), PQ, H1p, H1, H2, gout, ldg, saved,
                                          W2Tp, H2p, plan, dpre_c, dpre_ovf, dP, ldp, S(stream));
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_bwd_compact", "shape outside the compact envelope (gn_edgeconv_dpre_compact_supported)");
    if (r == hipErrorInvalidValue) return bad("gn_edgeconv_bwd_compact", "H1p%32, H2p%32, 16-byte row pitches");
    return fail(r, "gn_edgeconv_bwd_compact");
}
int gn_edgeconv_dq_gather_compact(int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2, const void* saved, const void* plan,
                                  const void* dpre_c, const void* dpre_ovf, const int32_t* rev_ptr, const int32_t* rev_rows,
                                  const int32_t* hubs, const int32_t* nhubs, void* dQ, int64_t ldq, void* stream) {
    if (K < 1 || K > 16 || !saved || !plan || !dpre_c) return bad("gn_edgeconv_dq_gather_compact", "need 1<=K<=16, saved, plan, dpre_c");
    hipError_t r = gn::launch_dq_gather_cp_saved(N, K, H1p, H1, H2, saved, plan, dpre_c, dpre_ovf, rev_ptr, rev_rows, hubs, nhubs,
                                                 dQ, ldq, S(stream));
    if (r == hipErrorNotSupported) return bad("gn_edgeconv_dq_gather_compact", "shape outside the compact envelope");
    if (r == hipErrorInvalidValue) return bad("gn_edgeconv_dq_gather_compact", "16-byte dQ row pitch");
    return fail(r, "gn_edgeconv_dq_gather_compact");
}

int gn_edgeconv_dq_gather(int32_t mode, const void* dpre, int32_t H1p, const int32_t* rev_ptr, const int32_t* rev_rows,
                          const int32_t* hubs, const int32_t* nhubs, int32_t N, void* dQ, int64_t ldq, void* stream) {
    hipError_t r = gn::launch_dq_gather(mode, dpre, H1p, rev_ptr, rev_rows, hubs, nhubs, N, dQ, ldq, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_edgeconv_dq_gather", "need H1p <= 512, H1p%8==0, 16-byte dQ row pitch");
    return fail(r, "gn_edgeconv_dq_gather");
}

int gn_edge_rows(const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src, const int32_t* ovf_cnt, int32_t N,
                 int32_t K, int32_t* ic, int32_t* jc, void* stream) {
    if (K < 1 || K > 32) return bad("gn_edge_rows", "need 1<=K<=32");
    return fail(gn::launch_edge_rows(make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), gn::edge_slots(K), ic, jc,
                                     S(stream)), "gn_edge_rows");
}
int gn_rows_compact(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, int32_t* deg, int32_t* tmp, int32_t* row_ptr,
                    int32_t* ic, int32_t* jc, void* stream) {
    if (K < 1 || K > 32) return bad("gn_rows_compact", "need 1<=K<=32");
    return fail(gn::launch_rows_compact(make_graph(nbr, nullptr, nullptr, nullptr, N, K), ovf, deg, tmp, row_ptr, ic, jc, S(stream)),
                "gn_rows_compact");
}
int gn_segment_rows_sum(const float* m, int64_t ldm, int32_t C, int32_t N, const int32_t* row_ptr, float* out, int64_t ldo, int32_t m_lowp,
                        void* stream) {
    hipError_t r = gn::launch_segment_rows_sum(m, ldm, C, N, row_ptr, out, ldo, m_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_segment_rows_sum", "need C >= 1");
    return fail(r, "gn_segment_rows_sum");
}
int gn_rev_rows_compact(const int32_t* nbr, const int32_t* ovf_centre, int32_t N, int32_t K, const int32_t* row_ptr,
                        const int32_t* rev_ptr, const int32_t* rev_rows, int32_t* out, void* stream) {
    if (K < 1 || K > 32) return bad("gn_rev_rows_compact", "need 1<=K<=32");
    return fail(gn::launch_rev_rows_compact(make_graph(nbr, ovf_centre, nullptr, nullptr, N, K), gn::edge_slots(K), row_ptr, rev_ptr,
                                            rev_rows, out, S(stream)), "gn_rev_rows_compact");
}
int gn_edge_gather_pre(const float* PQ, int32_t H1p, const int32_t* ic, const int32_t* jc, int64_t rows, int32_t act,
                       void* pre, int32_t pre_lowp, void* stream) {
    hipError_t r = gn::launch_edge_gather_pre(PQ, H1p, ic, jc, rows, act, pre, pre_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_edge_gather_pre", "H1p % 4 (bf16: % 8) != 0, or act not in {2 leaky relu, 3 identity}");
    return fail(r, "gn_edge_gather_pre");
}
int gn_rownorm_act_fwd(const float* z, int64_t ldz, int32_t C, const int32_t* valid, const float* gamma, const float* beta,
                       float eps, int32_t act, float* a, int64_t lda, int32_t Cpad, float* stats, int64_t rows,
                       void* a_bf16, int64_t lda_bf16, int32_t z_lowp, void* stream) {
    if (!a && !a_bf16) return bad("gn_rownorm_act_fwd", "a and / or a_bf16");
    hipError_t r = gn::launch_rownorm_act_fwd(z, ldz, C, valid, gamma, beta, eps, act, a, lda, Cpad, stats, rows, a_bf16,
                                              lda_bf16, z_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_rownorm_act_fwd", "need 1 <= C <= Cpad <= 512, act in 0..3, gamma and beta together");
    return fail(r, "gn_rownorm_act_fwd");
}
int32_t gn_rownorm_bwd_blocks(int64_t rows) { return gn::rownorm_bwd_blocks(rows); }
int gn_rownorm_act_bwd(const float* g, int64_t ldg, const int32_t* gidx, const float* z, int64_t ldz, int32_t C,
                       const int32_t* valid, const float* gamma, const float* beta, const float* stats, int32_t act,
                       float* dz, int64_t lddz, int32_t Cpad, float* t_dy, float* t_dyx, int64_t rows, void* dz_bf16,
                       int64_t lddz_bf16, const int32_t* argrow, int32_t z_lowp, void* stream) {
    if (!dz && !dz_bf16) return bad("gn_rownorm_act_bwd", "dz and / or dz_bf16");
    hipError_t r = gn::launch_rownorm_act_bwd(g, ldg, gidx, z, ldz, C, valid, gamma, beta, stats, act, dz, lddz, Cpad, t_dy,
                                              t_dyx, rows, dz_bf16, lddz_bf16, argrow, z_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_rownorm_act_bwd", "need 1 <= C <= Cpad <= 512, act in 0..3; LayerNorm needs beta, stats, t_dy, t_dyx");
    return fail(r, "gn_rownorm_act_bwd");
}
int gn_slot_sum(const float* m, int64_t ldm, int32_t C, const int32_t* nbr, const int32_t* ovf_centre,
                const int32_t* ovf_src, const int32_t* ovf_cnt, int32_t N, int32_t K, float* out, int64_t ldo,
                void* stream) {
    if (K < 1 || K > 32) return bad("gn_slot_sum", "need 1<=K<=32");
    return fail(gn::launch_slot_sum(m, ldm, C, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), gn::edge_slots(K), out,
                                    ldo, S(stream)), "gn_slot_sum");
}

int gn_slot_reduce(const float* m, int64_t ldm, int32_t C, const int32_t* nbr, const int32_t* ovf_centre,
                   const int32_t* ovf_src, const int32_t* ovf_cnt, int32_t N, int32_t K, const int32_t* jc, int32_t aggr,
                   float* out, int64_t ldo, int32_t* ovf_row, int32_t* deg, int32_t* argrow, int32_t post_act, void* stream) {
    if (K < 1 || K > 32) return bad("gn_slot_reduce", "need 1<=K<=32");
    hipError_t r = gn::launch_slot_reduce(m, ldm, C, make_graph(nbr, ovf_centre, ovf_src, ovf_cnt, N, K), gn::edge_slots(K),
                                          jc, aggr, out, ldo, ovf_row, deg, argrow, post_act, S(stream));
    if (r == hipErrorInvalidValue)
        return bad("gn_slot_reduce", "aggr in 0..2, ovf_row / deg required, argrow for max, post_act 3 (none) or 2 (leaky relu, max only)");
    return fail(r, "gn_slot_reduce");
}
int gn_slot_reduce_bwd(const float* gout, int64_t ldg, int32_t C, const int32_t* ic, const int32_t* jc, int64_t rows,
                       int32_t aggr, const int32_t* deg, const int32_t* argrow, float* grows, int64_t ldr, int32_t Cpad,
                       void* stream) {
    hipError_t r = gn::launch_slot_reduce_bwd(gout, ldg, C, ic, jc, rows, aggr, deg, argrow, grows, ldr, Cpad, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_slot_reduce_bwd", "aggr in 0..2, deg for mean, argrow for max, Cpad >= C");
    return fail(r, "gn_slot_reduce_bwd");
}

int gn_pack_weights(const int64_t* desc, int32_t ndesc, void* stream) {
    if (ndesc < 0 || (ndesc > 0 && !desc)) return bad("gn_pack_weights", "descriptor table");
    return fail(gn::launch_pack_weights(reinterpret_cast<const long long*>(desc), ndesc, S(stream)), "gn_pack_weights");
}

int gn_segment_pool_fwd(const float* x, int64_t ldx, int32_t C, const int32_t* ptr, int32_t B, const int32_t* codes_host,
                        int32_t ns, float* out, int32_t* argmin, int32_t* argmax, void* stream) {
    hipError_t r = gn::launch_pool_fwd(x, ldx, C, ptr, B, 0, codes_host, ns, out, argmin, argmax, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_segment_pool_fwd", "1..4 pooling schemes");
    return fail(r, "gn_segment_pool_fwd");
}
int gn_segment_pool_fwd_ws(const float* x, int64_t ldx, int32_t C, const int32_t* ptr, int32_t B, int32_t N, const int32_t* codes_host,
                           int32_t ns, float* out, int32_t* argmin, int32_t* argmax, void* scratch, void* stream) {
    hipError_t r = gn::launch_pool_fwd(x, ldx, C, ptr, B, N, codes_host, ns, out, argmin, argmax, S(stream), scratch);
    if (r == hipErrorInvalidValue) return bad("gn_segment_pool_fwd", "1..4 pooling schemes");
    return fail(r, "gn_segment_pool_fwd");
}
int gn_segment_pool_bwd(const float* gout, int32_t C, const int32_t* ptr, const int32_t* batch, int32_t N,
                        const int32_t* codes_host, int32_t ns, const int32_t* argmin, const int32_t* argmax,
                        const float* gate, int64_t ldgate, void* dx, int64_t lddx, int32_t dx_lowp, void* stream) {
    hipError_t r = gn::launch_pool_bwd(gout, C, ptr, batch, N, codes_host, ns, argmin, argmax, gate, ldgate, dx, lddx,
                                       dx_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_segment_pool_bwd", "1..4 pooling schemes");
    return fail(r, "gn_segment_pool_bwd");
}


int gn_attention_plan(const int32_t* ptr, int32_t B, int32_t* plan, int32_t sorted, void* stream) {
    hipError_t r = gn::launch_attn_plan(ptr, B, plan, sorted, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_attention_plan", "B >= 0");
    return fail(r, "gn_attention_plan");
}
int gn_attention_fwd(int32_t lowp, const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr,
                     const int32_t* tile_ptr, int32_t B, int32_t N, void* out, int64_t ldo, float* lse2, uint32_t drop_seed,
                     uint32_t drop_thresh, void* stream) {
    if (H <= 0 || B < 0 || N < 0) return bad("gn_attention_fwd", "H > 0, B >= 0, N >= 0");
    hipError_t r = gn::launch_attn_fwd(lowp, qkv, ld, H, DH, ptr, tile_ptr, B, N, out, ldo, lse2, drop_seed, drop_thresh,
                                       nullptr, nullptr, nullptr, 0, S(stream));
    if (r == hipErrorInvalidValue)
        return bad("gn_attention_fwd", "head width in {8,16,32,64} (fp32) or {32,64} (bf16), row pitches multiples of 16 bytes");
    return fail(r, "gn_attention_fwd");
}
int gn_attention_fwd_bits(const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr,
                          int32_t B, int32_t N, void* out, int64_t ldo, float* lse2, uint32_t drop_seed, uint32_t drop_thresh,
                          uint32_t* bits_r, uint32_t* bits_c, const int64_t* evoff, int64_t plane_words, void* stream) {
    if (H <= 0 || B < 0 || N < 0 || !bits_r || !bits_c || !evoff || plane_words < 0 || drop_thresh == 0)
        return bad("gn_attention_fwd_bits", "H > 0, B >= 0, N >= 0, drop_thresh != 0, bit planes and event offsets given");
    hipError_t r = gn::launch_attn_fwd(1, qkv, ld, H, DH, ptr, tile_ptr, B, N, out, ldo, lse2, drop_seed, drop_thresh, bits_r,
                                       bits_c, reinterpret_cast<const long long*>(evoff), plane_words, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_attention_fwd_bits", "head width in {32,64}, row pitches multiples of 16 bytes");
    return fail(r, "gn_attention_fwd_bits");
}
int gn_attention_bwd(int32_t lowp, const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr,
                     const int32_t* tile_ptr, int32_t B, int32_t N, const void* out, int64_t ldo, const void* dout,
                     int64_t lddo, const float* lse2, float* delta, void* dqkv, int64_t lddq, uint32_t drop_seed,
                     uint32_t drop_thresh, void* stream) {
    if (H <= 0 || B < 0 || N < 0) return bad("gn_attention_bwd", "H > 0, B >= 0, N >= 0");
    hipError_t r = gn::launch_attn_bwd(lowp, qkv, ld, H, DH, ptr, tile_ptr, B, N, out, ldo, dout, lddo, lse2, delta, dqkv,
                                       lddq, drop_seed, drop_thresh, nullptr, nullptr, nullptr, 0, S(stream));
    if (r == hipErrorInvalidValue)
        return bad("gn_attention_bwd", "head width in {8,16,32,64} (fp32) or {32,64} (bf16), row pitches multiples of 16 bytes");
    return fail(r, "gn_attention_bwd");
}
int gn_attention_bwd_bits(const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr,
                          int32_t B, int32_t N, const void* out, int64_t ldo, const void* dout, int64_t lddo, const float* lse2,
                          float* delta, void* dqkv, int64_t lddq, uint32_t drop_thresh, const uint32_t* bits_r,
                          const uint32_t* bits_c, const int64_t* evoff, int64_t plane_words, void* stream) {
    if (H <= 0 || B < 0 || N < 0 || !bits_r || !bits_c || !evoff || plane_words < 0 || drop_thresh == 0)
        return bad("gn_attention_bwd_bits", "H > 0, B >= 0, N >= 0, drop_thresh != 0, bit planes and event offsets given");
    hipError_t r = gn::launch_attn_bwd(1, qkv, ld, H, DH, ptr, tile_ptr, B, N, out, ldo, dout, lddo, lse2, delta, dqkv, lddq, 0u,
                                       drop_thresh, bits_r, bits_c, reinterpret_cast<const long long*>(evoff), plane_words,
                                       S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_attention_bwd_bits", "head width in {32,64}, row pitches multiples of 16 bytes");
    return fail(r, "gn_attention_bwd_bits");
}

int gn_rel_attention_supported(int32_t DH) { return gn::rel_attn_supported(DH) ? 1 : 0; }
int gn_rel_attention_fwd(const float* qkv, int64_t ld, const float* qp, int64_t ldqp, const float* xt, int64_t ldxt,
                         const float* freq, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr, int32_t B,
                         int32_t N, float* out, int64_t ldo, float* u, int64_t ldu, float* lse2, void* stream) {
    if (H <= 0 || B < 0 || N < 0) return bad("gn_rel_attention_fwd", "H > 0, B >= 0, N >= 0");
    if (N > 0 && B > 0 && (!qkv || !qp || !xt || !freq || !ptr || !tile_ptr || !out || !u || !lse2))
        return bad("gn_rel_attention_fwd", "null pointer");
    hipError_t r = gn::launch_rel_attn_fwd(qkv, ld, qp, ldqp, xt, ldxt, freq, H, DH, ptr, tile_ptr, B, N, out, ldo, u, ldu, lse2,
                                           S(stream));
    if (r == hipErrorInvalidValue)
        return bad("gn_rel_attention_fwd", "head width 32, row pitches multiples of 16 bytes and at least the row width, xt pitch >= 4");
    return fail(r, "gn_rel_attention_fwd");
}
int gn_rel_attention_bwd(const float* qkv, int64_t ld, const float* qp, int64_t ldqp, const float* xt, int64_t ldxt,
                         const float* freq, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr, int32_t B,
                         int32_t N, const float* out, int64_t ldo, const float* u, int64_t ldu, const float* dout,
                         int64_t lddo, const float* du, int64_t lddu, const float* lse2, float* delta, float* dqkv,
                         int64_t lddq, float* dqp, int64_t lddqp, void* stream) {
    if (H <= 0 || B < 0 || N < 0) return bad("gn_rel_attention_bwd", "H > 0, B >= 0, N >= 0");
    if (N > 0 && B > 0 && (!qkv || !qp || !xt || !freq || !ptr || !tile_ptr || !out || !u || !dout || !du || !lse2 || !delta ||
                           !dqkv || !dqp))
        return bad("gn_rel_attention_bwd", "null pointer");
    hipError_t r = gn::launch_rel_attn_bwd(qkv, ld, qp, ldqp, xt, ldxt, freq, H, DH, ptr, tile_ptr, B, N, out, ldo, u, ldu, dout,
                                           lddo, du, lddu, lse2, delta, dqkv, lddq, dqp, lddqp, S(stream));
    if (r == hipErrorInvalidValue)
        return bad("gn_rel_attention_bwd", "head width 32, row pitches multiples of 16 bytes and at least the row width, xt pitch >= 4");
    return fail(r, "gn_rel_attention_bwd");
}

int gn_dropout(const void* x, int64_t ldx, int32_t x_lowp, const float* res, int64_t ldres, void* y, int64_t ldy,
               int32_t y_lowp, int64_t rows, int32_t cols, uint32_t seed, uint32_t thresh, void* stream) {
    hipError_t r = gn::launch_dropout(x, ldx, x_lowp, res, ldres, y, ldy, y_lowp, rows, cols, seed, thresh, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_dropout", "cols and row pitches multiples of 4");
    return fail(r, "gn_dropout");
}


int64_t gn_bn_blocks(int64_t rows) { return gn::bn_blocks(rows); }
int gn_bn_sums(int32_t mode, int32_t act, const float* z, int64_t ldz, int64_t rows, int32_t C, const int32_t* valid,
               const float* g, int64_t ldg, const float* mean, const float* rstd, const float* gamma, const float* beta,
               float* part, float* sums, void* stream) {
    hipError_t r = gn::launch_bn_sums(mode, act, z, ldz, rows, C, valid, g, ldg, mean, rstd, gamma, beta, part, sums, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_bn_sums", "1 <= C <= 512, mode 0 / 1, act 0..3");
    return fail(r, "gn_bn_sums");
}
int gn_bn_finalize(const float* sums, const int32_t* n_valid, int32_t C, float eps, float* mean, float* rstd,
                   float* var_unbiased, void* stream) {
    return fail(gn::launch_bn_finalize(sums, n_valid, C, eps, mean, rstd, var_unbiased, S(stream)), "gn_bn_finalize");
}
int gn_bn_act_fwd(const float* z, int64_t ldz, int64_t rows, int32_t C, const int32_t* valid, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, int32_t act, void* a, int64_t lda, int32_t Cpad,
                  int32_t a_lowp, void* stream) {
    hipError_t r = gn::launch_bn_act_fwd(z, ldz, rows, C, valid, mean, rstd, gamma, beta, act, a, lda, Cpad, a_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_bn_act_fwd", "1 <= C <= Cpad, Cpad % 4 == 0, act 0..3");
    return fail(r, "gn_bn_act_fwd");
}
int gn_bn_act_bwd(const float* g, int64_t ldg, const float* z, int64_t ldz, int64_t rows, int32_t C, const int32_t* valid,
                  const float* mean, const float* rstd, const float* gamma, const float* beta, const float* sums,
                  const int32_t* n_valid, int32_t act, void* dz, int64_t lddz, int32_t Cpad, int32_t dz_lowp, void* stream) {
    hipError_t r = gn::launch_bn_act_bwd(g, ldg, z, ldz, rows, C, valid, mean, rstd, gamma, beta, sums, n_valid, act, dz, lddz,
                                         Cpad, dz_lowp, S(stream));
    if (r == hipErrorInvalidValue) return bad("gn_bn_act_bwd", "1 <= C <= Cpad, Cpad % 4 == 0, act 0..3, n_valid with sums");
    return fail(r, "gn_bn_act_bwd");
}

}  // extern "C"
