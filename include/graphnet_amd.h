/*
 * include/graphnet_amd.h — C ABI of libgraphnet_amd.so (hand-written gfx950 HIP kernels).
 *
 * Drop-in boundary for the DynEdge message-passing path of graphnet.  The reference has no
 * FFI of its own (pure Python): its plugin boundary is the Python class
 * GNN (src/graphnet/models/gnn/gnn.py:11-35) and the third-party operators it calls.
 * Each entry point below names the reference call site / third-party operator it replaces.
 * Host-side binding: graphnet_amd/_lib.py (ctypes); see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the comment says "host";
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued, nothing synchronises;
 *   - return value: 0 on success, otherwise a hipError_t code; gn_last_error() has the text;
 *   - mode: 0 = f32 operands (v_mfma_f32_32x32x2_f32, parity mode), 1 = bf16 operands
 *     (v_mfma_f32_32x32x16_bf16); accumulation is fp32 in both; "T" below is float or bf16;
 *   - activations and their gradients between the kernels ("act" tensors: x0, conv outputs, dPQ,
 *     d_out, post-MLP hidden layers) are T: fp32 in mode 0, bf16 in mode 1 (a GEMM would round them
 *     to bf16 on load anyway, so keeping them as bf16 in HBM halves the bytes without changing a
 *     result); k-NN coordinates, the last post-MLP output (pooling input), pooled features,
 *     weights, biases and every weight gradient stay fp32 in both modes;
 *   - layout: batched CSR — x[N, ld] row-major fp32, ptr[B+1] int32 event offsets,
 *     batch[N] int32 event ids, neighbour table nbr[N, K] int32 (-1 padded) + overflow list.
 */
#ifndef GRAPHNET_AMD_H
#define GRAPHNET_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GN_MODE_F32 0
#define GN_MODE_BF16 1
#define GN_MAXSEG 6

const char* gn_last_error(void);
#define GN_ABI_VERSION 7   /* 7: gn_knn_graph_ws (sorted sweep of large events), gn_rev_build_events_ws, gn_*_ws event reductions, compact edge rows; 6: gn_edgeconv_leaky_* (DynEdgeJINST), `saved` gains the row-validity words, gn_edgeconv_dw2_reduce;
                              2: gn_edgeconv_fwd takes the real hidden width H1; 3: gn_edgeconv_max_* (EdgeConvTito); 4: gn_attention_*_bits;
                              5: gn_dynedge_fwd / gn_dynedge_bwd (one entry per backbone pass), gn_edgeconv_saved_offsets, compact dpre */
int gn_abi_version(void);   /* == GN_ABI_VERSION of the header the library was built from */

/* ---- graph construction ------------------------------------------------------------- */

/* torch_geometric.nn.knn_graph(x[:, cols], k, batch) as called at
 * models/graphs/edges/edges.py:74-78 and models/components/layers.py:63-67.
 * cols: HOST int[D] (D <= 8).  strict = 0: k+1-with-self then mask (degree k or k+1, the extra
 * neighbour goes to ovf[N], -1 if none); strict = 1: self excluded, ovf may be NULL. */
int gn_knn_graph(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D,
                 const int32_t* ptr, const int32_t* tile_ptr, int32_t B, int32_t N, int32_t k, int32_t strict,
                 int32_t* nbr, int32_t* ovf, void* stream);
/* The same table with scratch for the large-event path: events of 1025..16384 pulses, in batches that average >= 512 pulses per
 * event (BASELINE configs[4]: 10^4 pulses per event), are sorted along a space-filling curve and scanned with bounding-box
 * pruning instead of exhaustively - the lists are identical entry for entry.  ws: gn_knn_ws_bytes(B, N, D) bytes, 256-byte
 * aligned, or NULL (= gn_knn_graph). */
int64_t gn_knn_ws_bytes(int32_t B, int32_t N, int32_t D);
int gn_knn_graph_ws(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D,
                    const int32_t* ptr, const int32_t* tile_ptr, int32_t B, int32_t N, int32_t k, int32_t strict,
                    int32_t* nbr, int32_t* ovf, void* ws, void* stream);
/* Query-tile plan of a batch (once per batch, shared by every k-NN layer).  Device int32[2B + 2 + N/64]:
 * tile_ptr[e] = number of 64-query tiles of the events before e, tile_ptr[B] = their total (<= N/64 + B),
 * tile_ptr[B+1] = number of tiles that belong to events above 1024 pulses, their ids from tile_ptr[B+2]
 * (those tiles are scanned by 8 waves each, the others by one). */
int gn_knn_plan(const int32_t* ptr, int32_t B, int32_t* tile_ptr, void* stream);
/* MinkowskiKNNEdges (models/graphs/edges/minkowski.py:66-99), per centre: among the pulses j != i of its own event the k
 * smallest in the total order (m, j), fp32 without FMA contraction:
 *   sp = ((0 + d0*d0) + d1*d1) + ... over space_cols;  tc = (t_i - t_j) * c;  m = sp - tc*tc;
 *   if (m < 0) m = m * (-time_like_weight)
 * The query is excluded by index; a NaN m or m >= 3.0e38f is nobody's neighbour.  nbr[N, k]: the strict table (degree
 * min(k, n - 1), ascending (m, j), -1 padded, no overflow column).  space_cols: HOST int[DS], 1 <= DS <= 7; every column
 * < ldx; 1 <= k <= 32; tile_ptr: the plan of gn_knn_plan.  Events of any size are scanned exhaustively. */
int gn_minkowski_knn_graph(const float* x, int64_t ldx, const int32_t* space_cols_host, int32_t DS, int32_t time_col,
                           float c, float time_like_weight, const int32_t* ptr, const int32_t* tile_ptr,
                           int32_t B, int32_t N, int32_t k, int32_t* nbr, void* stream);
/* RadialEdges (models/graphs/edges/edges.py:83-117; radius_graph with max_num_neighbors = cap): edge j -> i iff j != i,
 * both in one event, and d2 < r2 (strict), fp32 without FMA contraction:
 *   d2 = ((0 + e0*e0) + e1*e1) + ...  e = x[j, col] - x[i, col], columns left to right;  r2 = r * r (one fp32 multiply)
 * The centre is excluded by index; a pulse with a NaN or inf coordinate has no neighbours and is nobody's neighbour.
 * nbr[N, cap]: every centre's sources ascending by j, -1 padded; a centre with more than cap in-radius pulses keeps the cap
 * smallest in the total order (d2, j), still stored ascending by j.  deg[N]: the UNCAPPED in-radius count.
 * cols: HOST int[D], 1 <= D <= 8, every column < ldx; 1 <= cap <= 32; r finite and > 0; tile_ptr: the plan of gn_knn_plan
 * (required); work: gn_radius_work_ints(B, N) ints of scratch.  Events of any size are scanned exhaustively. */
int64_t gn_radius_work_ints(int32_t B, int32_t N);
int gn_radius_graph(const float* x, int64_t ldx, const int32_t* cols_host, int32_t D, float r, const int32_t* ptr,
                    const int32_t* tile_ptr, int32_t B, int32_t N, int32_t cap, int32_t* nbr, int32_t* deg, int32_t* work,
                    void* stream);

/* PercentileClusters (models/graphs/nodes/nodes.py:135-217): one node per distinct tuple of the cluster columns inside each
 * event, every summarised column reduced to P percentiles, fp32 in and out.
 *   key of a cluster value: its fp32 bits with -0.0 taken as +0.0 and every NaN as ONE value after +inf; two pulses share a
 *     cluster iff all C keys are equal (NaNs cluster together: a definition).
 *   row order: clusters ascend lexicographically, the LAST cluster column most significant (np.lexsort of the columns).
 *   row = [x[first, c_0 .. c_{C-1}] | for f in summ_cols, for p: pct(f, p) | log10(count) if add_counts], first = the
 *     lowest-index pulse of the cluster, W = C + S*P + add_counts columns.
 *   pct: v[0..m) = the cluster's non-NaN values of f, ascending, as fp64 (m = 0 -> NaN); fp64 without FMA contraction:
 *     h = (m-1)*q; lo = floor(h); hi = min(lo+1, m-1); g = h - lo; d = v[hi] - v[lo];
 *     r = g >= 0.5 ? v[hi] - d*(1-g) : v[lo] + d*g;  out = (float) r        (numpy's method "linear"; q = percentile / 100)
 *   count: pulses of the cluster (NaN values included); the column is (float) log10((double) count), exactly 0 for 1.
 * out[N, ldo]: room for N rows (never more clusters than pulses), the first out_ptr[B] are written; out_ptr[B+1]: cluster
 * offsets per event, out_ptr[B] = node count.  cluster_cols / summ_cols / q: HOST arrays; 1 <= C <= 8, 1 <= S <= 32,
 * 1 <= P <= 16, 0 <= q <= 1, columns distinct and < ldx, ldo >= W, N <= 2^28.  work: gn_percentile_work_ints(B, N) ints, 8-byte
 * aligned.  Events of up to gn_percentile_lds_max() pulses sort in LDS, larger ones in `work` (correct, not fast). */
int64_t gn_percentile_work_ints(int32_t B, int32_t N);
int32_t gn_percentile_lds_max(void);   /* largest event sorted in LDS */
int gn_percentile_clusters(const float* x, int64_t ldx, int32_t N, const int32_t* ptr, int32_t B,
                           const int32_t* cluster_cols_host, int32_t C, const int32_t* summ_cols_host, int32_t S,
                           const double* q_host, int32_t P, int32_t add_counts,
                           float* out, int64_t ldo, int32_t* out_ptr, int32_t* work, void* stream);

/* NodeAsDOMTimeSeries (models/graphs/nodes/nodes.py:220-306): the pulses of each event regrouped into one time series per
 * DOM; the row count does not change.  x[N, ldx] with F feature columns, fp32 in and out, out must not overlap x; ptr[B+1]
 * with ptr[0] = 0 and ptr[B] = N.  Per event:
 *   row order: ONE stable sort of the event's rows.  Keys, most significant first: the id columns in np.lexsort order (the
 *     LAST of id_cols most significant), then the time column ascending, then the original pulse index.  Id keys are those of
 *     gn_percentile_clusters (-0.0 taken as +0.0, every NaN one value after +inf); the time key likewise takes -0.0 as +0.0
 *     and puts NaN last, as argsort does.  (The reference runs an unstable argsort on time and then a stable lexsort: the
 *     order among equal times of one DOM is a definition of this library.)  Done as C + 1 stable passes, time first.
 *   time column: x - tmin, one fp32 subtraction; tmin = the event's smallest time (-0.0 before +0.0), or NaN if any time of
 *     the event is NaN (numpy's min propagates it), which makes the whole column NaN.
 *   charge column: (float) pow(10.0, (double) v), undoing the detector's log10.  charge_col = -1: no such column; a column
 *     of exactly 1.0f is appended at index F (the reference inserts zeros and raises 10 to them).
 *   last column, new_node_col: 1.0f on the first row of every id tuple of the event, 0.0f elsewhere.
 *   W = F + (charge_col < 0) + 1 columns; every other column is copied bit for bit.
 * series_ptr, int32 with room for N + 1: the batch row at which each of the M series starts, then N.  dom_ptr[B+1]: series
 * offsets per event, dom_ptr[B] = M.  An empty batch writes series_ptr[0] = 0; empty events are legal.
 * id_cols: HOST int[C], 1 <= C <= 8; id, time and charge columns distinct and < F <= ldx; ldo >= W; N <= 2^28.
 * work: gn_dom_time_series_work_ints(B, N) ints, 8-byte aligned.  Events of up to gn_percentile_lds_max() pulses sort in
 * LDS, larger ones in `work` (correct, not fast). */
int64_t gn_dom_time_series_work_ints(int32_t B, int32_t N);
int gn_dom_time_series(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* ptr, int32_t B,
                       const int32_t* id_cols_host, int32_t C, int32_t time_col, int32_t charge_col,
                       float* out, int64_t ldo, int32_t* series_ptr, int32_t* dom_ptr, int32_t* work, void* stream);

/* IceMixNodes (models/graphs/nodes/nodes.py:309-453): every event cut to at most L = max_pulses of its pulses, the hlc column
 * flipped, two ice columns interpolated from a table.  x[N, ldx] with F feature columns, fp32 in and out, out must not overlap
 * x; ptr[B+1] ascending with ptr[0] = 0 and ptr[B] = N; empty events are legal.  Per event b with n pulses:
 *   key of pulse i (its index INSIDE the event): stream e = event_ids ? event_ids[b] : b (uint32), and
 *     h = gn_mix32(gn_mix32(seed ^ e*0x9E3779B1) ^ i*0x85EBCA77) >> (32 - key_bits)         all in uint32 arithmetic;
 *     gn_mix32(v): v ^= v >> 16; v *= 0x21F0AAAD; v ^= v >> 15; v *= 0x735A2D97; v ^= v >> 15   (the dropout hash, (a, b) = (e, i)).
 *   selection: n <= L keeps every pulse; otherwise pulse i is kept iff fewer than L pulses of the event precede it in the
 *     total order (h, i).  Rows are written in ascending i in both cases.  (The reference draws randperm(n) and indexes it at
 *     the flagged positions, which is a uniformly random L-subset whatever the hlc column holds, sorted when there is an hlc
 *     column and in random order when there is none; the contract here is that distribution, always ascending, and not
 *     torch's generator stream.)  key_bits is 32 in production; fewer bits force equal keys, for tests of the tie rule.
 *   row of kept pulse id (a row of x): out[., c] = x[id, c] bit for bit for c < F, but
 *     c == hlc_col: x[id, c] == 0 ? 1.0f : 0.0f     (logical_not; a NaN gives 0);
 *     z_col >= 0: two more columns, F (scattering) and F + 1 (absorption), from table = zt[T] | ys[T] | ya[T] (doubles, zt
 *       strictly ascending, ys / ya already scaled).  z = (double) x[id, z_col]; j = the largest index with zt[j] <= z, at
 *       most T - 2 (so z == zt[T-1] lies in the last interval); fp64, one rounding per operation, no FMA contraction:
 *         slope = (y[j+1] - y[j]) / (zt[j+1] - zt[j]);  v = slope * (z - zt[j]) + y[j];  out = (float) v
 *       z < zt[0], z > zt[T-1] or NaN: NaN in both columns (a kernel cannot raise; the host path of the package does).
 *   W = F + 2*(z_col >= 0) columns.
 * out[M, ldo] and ids[M], M = sum_b min(n_b, L) <= N (room for N rows always suffices; nothing is written past row N - 1);
 * out_ptr[B+1]: row offsets per event, out_ptr[B] = M; ids[r]: the row of x that output row r came from.
 * table: DEVICE pointer (unused with z_col = -1), 2 <= T <= 1024; event_ids: DEVICE uint32[B] or NULL; hlc_col / z_col < F
 * (-1: none); max_pulses >= 1; 1 <= key_bits <= 32; ldo >= W; N <= 2^28.  No work buffer and no limit on the size of an
 * event; integer LDS atomics only: two runs agree bit for bit. */
int gn_icemix_nodes(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* ptr, int32_t B, int32_t max_pulses,
                    int32_t hlc_col, int32_t z_col, const double* table, int32_t T, uint32_t seed, const uint32_t* event_ids,
                    int32_t key_bits, float* out, int64_t ldo, int32_t* out_ptr, int32_t* ids, void* stream);

/* Ragged GRU recurrence over series(models/rnn/node_rnn.py:105-111; layer 0 of torch.nn.GRU).  Series s owns rows
 * series_ptr[s] .. series_ptr[s+1] of xs[T, ldx] (I columns); series_ptr[0] = 0, series_ptr[M] = T, no empty series.  Gate
 * order and tensors are torch.nn.GRU's: r, z, n; weight_ih[3H, I], weight_hh[3H, H], bias_ih[3H], bias_hh[3H], contiguous.
 * h = 0, then for every row t of the series
 *   gi = W_ih x_t + b_ih;  gh = W_hh h + b_hh;  r = sigmoid(gi_r + gh_r);  z = sigmoid(gi_z + gh_z);
 *   n = tanh(gi_n + r * gh_n);  h = (1 - z) * n + z * h
 * and out[s, 0..H) = h after the last row.  fp32 whatever the compute mode of the other entries; sums in a fixed order, no
 * float atomics: two runs on one input agree bit for bit.
 * Envelope (gn_gru_supported(I, H) == 1): 1 <= I <= 32, 4 <= H <= 64, H a multiple of 4.  Outside it the entries fail.
 * saved (null for inference): gn_gru_saved_floats(T, H) = 5*T*H floats, 16-byte aligned: planes [T, H] of r, z, n, gh_n and
 * h_prev (zeros on a series' first row).
 * gn_gru_series_bwd: dout[M, H] -> dw_ih[3H, Ip] (Ip = I rounded up to a multiple of 4; the padding columns are 0),
 * db_ih[3H], dw_hh[3H, H], db_hh[3H], overwritten.  xs gets no gradient.  work: gn_gru_bwd_work_floats(T, I, H) floats,
 * 16-byte aligned (the per-row pre-activation gradients and the split-reduction slabs of the four sums). */
int32_t gn_gru_supported(int32_t I, int32_t H);
int64_t gn_gru_saved_floats(int32_t T, int32_t H);
int64_t gn_gru_bwd_work_floats(int32_t T, int32_t I, int32_t H);
int gn_gru_series_fwd(const float* xs, int64_t ldx, int32_t T, int32_t I, const int32_t* series_ptr, int32_t M, int32_t H,
                      const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                      float* out, float* saved, void* stream);
int gn_gru_series_bwd(const float* dout, const float* saved, const float* xs, int64_t ldx, int32_t T, int32_t I,
                      const int32_t* series_ptr, int32_t M, int32_t H, const float* w_hh,
                      float* dw_ih, float* db_ih, float* dw_hh, float* db_hh, float* work, void* stream);
/* One row per series (node_rnn.py:113-122): out[s, 0..F) = x[series_ptr[s], 0..F), but column charge_col =
 * asinhf((5 * sum) / 5), sum = the fp32 sum of x[t, charge_col] over the series' rows in row order. */
int gn_dom_series_summary(const float* x, int64_t ldx, int32_t F, int32_t N, const int32_t* series_ptr, int32_t M,
                          int32_t charge_col, float* out, int64_t ldo, void* stream);

/* exclusive scan; tmp: >= gn_scan_tmp_ints(n) ints; total (optional) receives the sum */
int64_t gn_scan_tmp_ints(int64_t n);
int gn_scan_i32(const int32_t* in, int32_t* out, int32_t n, int32_t* tmp, int32_t* total, void* stream);

/* compact ovf[N] (>=0 entries) into ascending (ovf_centre, ovf_src) lists + device count */
int gn_ovf_compact(const int32_t* ovf, int32_t N, int32_t* work_N, int32_t* tmp,
                   int32_t* ovf_centre, int32_t* ovf_src, int32_t* ovf_cnt, void* stream);

/* reverse adjacency of the edge rows (row = i*S+slot, or N*S+t for overflow row t),
 * S = gn_edge_slots(K).  rev_ptr[N+1], cursor[N] scratch, rev_rows[>= N*K+N]. */
int32_t gn_edge_slots(int32_t K);
int gn_rev_build(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf_src, const int32_t* ovf_cnt,
                 int32_t* rev_ptr, int32_t* cursor, int32_t* tmp, int32_t* rev_rows, void* stream);
/* Same result for graphs whose edges never leave an event (what gn_knn_graph builds): one workgroup per event
 * counts, scans and fills with the in-degree counters in LDS.  ovf: per-centre overflow source ([N], -1 = none; the
 * array gn_knn_graph wrote) or NULL; ovf_pos[i]: index of centre i's overflow row (the exclusive scan gn_ovf_compact
 * leaves in its `work` array); ev: 2*(B+1) ints and scratch: N ints of workspace; hubs [N] / nhubs [1]: the hub list
 * for gn_edgeconv_dq_gather; tmp: gn_scan_tmp_ints(B) ints. */
/* An event's sources are cut into G = gn_rev_event_slices(B) slices, one workgroup each (a few huge events still
 * fill the chip): ev then holds 2*(B*G+1) ints and tmp gn_scan_tmp_ints(B*G) ints. */
int32_t gn_rev_event_slices(int32_t B);
int gn_rev_build_events(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf, const int32_t* ovf_pos,
                        const int32_t* ptr, int32_t B, int32_t* rev_ptr, int32_t* rev_rows, int32_t* ev,
                        int32_t* scratch, int32_t* hubs, int32_t* nhubs, int32_t* tmp, void* stream);

/* The same lists with scratch for batches of few, huge events (N >= 2048 * B, e.g. BASELINE configs[4]): the table is bucketed
 * by source slice first, so every entry is read twice instead of three times per slice of its event.  pairs:
 * gn_rev_pairs_ints(B, N, K) ints (0: this batch does not use it; pass NULL), or NULL (= gn_rev_build_events).  The lists
 * hold the same rows; their internal order is the order the atomics came in, in both entries. */
int64_t gn_rev_pairs_ints(int32_t B, int32_t N, int32_t K);
int gn_rev_build_events_ws(const int32_t* nbr, int32_t N, int32_t K, const int32_t* ovf, const int32_t* ovf_pos,
                           const int32_t* ptr, int32_t B, int32_t* rev_ptr, int32_t* rev_rows, int32_t* ev,
                           int32_t* scratch, int32_t* hubs, int32_t* nhubs, int32_t* tmp, int32_t* pairs, void* stream);

/* table <-> PyG edge_index[2,E] int64 (row 0 = source j, row 1 = target i, grouped by i) */
int gn_table_degree(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, int32_t* deg, void* stream);
int gn_table_to_edge_index(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, const int32_t* off,
                           int64_t E, int64_t* edge_index, void* stream);
/* gn_edge_index_to_table validates before it writes: *err (device int) comes back 0, or a mask of 1 = an index
 * outside [0, N) in either row, 2 = targets not ascending, 4 = an in-degree above K + 1; with bit 1 or 2 set the
 * table is left untouched (all -1).  The host side (ops.table_from_edge_index) sorts / re-sizes and calls again,
 * because PyG's EdgeConv (components/layers.py:60) accepts any edge order and degree. */
int gn_edge_index_to_table(const int64_t* edge_index, int64_t E, int32_t N, int32_t K, int32_t* first_N,
                           int32_t* nbr, int32_t* ovf, int32_t* err, void* stream);

int gn_ptr_to_batch(const int32_t* ptr, int32_t B, int32_t* batch, void* stream);

/* Detector._standardize (models/detector/detector.py:64-77; constants icecube.py:21-48, prometheus.py:11-39)
 * for the whole batch, in place: column f of x[N, ldx] runs nops_host[f] <= 3 steps, step k = op_host[3f+k]
 * (0 add, 1 sub, 2 mul, 3 div, 4 log10) with constant const_host[3f+k], fp32, no re-association.  HOST arrays. */
int gn_standardize(float* x, int64_t ldx, int32_t N, int32_t F, const int32_t* nops_host,
                   const int32_t* op_host, const float* const_host, void* stream);

/* DynEdge._calculate_global_variables (models/gnn/dynedge.py:266-293; homophily:
 * models/utils.py:13-29): out[B, F+5] = [mean_F | h_x h_y h_z h_t | log10 n_pulses] */
int gn_graph_globals(const float* x, int64_t ldx, int32_t F, const int32_t* ptr, int32_t B,
                     const int32_t* nbr, const int32_t* ovf, int32_t K, const int32_t* n_pulses,
                     float* out, void* stream);
/* gn_graph_globals / gn_segment_pool_fwd (below) for a batch of a FEW HUGE events (BASELINE configs[4]: 16 x 10^4 pulses: one
 * workgroup per event ran on 16 CUs).  Both reductions are DEFINED slice-wise: an event is reduced in slices of 1024
 * consecutive pulses that are folded in order, so an event's result never depends on its batch; the plain entries walk the
 * slices of an event in one workgroup.  With N (pulses in the batch) and a scratch buffer of gn_event_scratch_bytes(B, N, C)
 * bytes (C = pooled width; 0 for the global variables alone) a batch of <= 64 events runs one workgroup per slice and a
 * second small kernel folds them - the same operations in the same order, bit for bit.  scratch NULL: as the plain entries. */
int64_t gn_event_scratch_bytes(int32_t B, int32_t N, int32_t C);
int gn_graph_globals_ws(const float* x, int64_t ldx, int32_t F, const int32_t* ptr, int32_t B, int32_t N, const int32_t* nbr,
                        const int32_t* ovf, int32_t K, const int32_t* n_pulses, float* out, void* scratch, void* stream);
/* "distribute" + cat (dynedge.py:308-319) as a gather: x0[i] = [x[i] | gv[batch[i]] | 0-pad to ld0];
 * x0 is fp32, or bf16 when out_lowp */
int gn_concat_globals(const float* x, int64_t ldx, int32_t F, const float* gv, int32_t G,
                      const int32_t* batch, int32_t N, void* x0, int32_t ld0, int32_t out_lowp, void* stream);

/* ---- dense per-node layers (torch.nn.Linear at dynedge.py:198-231) -------------------- */

/* C[M, Nreal] = epi(sum_s A_s[M, width_s] . Wp[:, seg s]^T + bias); Wp: T[Npad][Kp] packed so
 * that segment s occupies kpad_s (multiple of 32) columns; A_s rows with pitch ld_s (elements), fp32 or
 * (a_lowp, mode 1) bf16 — widths/pitches multiples of 4 resp. 8, pad columns up to the multiple hold 0.
 * a_ptr/a_ld/a_width/a_kpad: HOST arrays of nseg entries.  gate: output *= (gate[m,n] > 0), fp32 or
 * (gate_lowp) bf16.  out_lowp: C is bf16 instead of fp32 (mode 1).  accum: C += (in C's own type). */
int gn_linear_fwd(int32_t mode, int32_t nseg, const void* const* a_ptr, int32_t a_lowp, const int64_t* a_ld,
                  const int32_t* a_width, const int32_t* a_kpad, int32_t M,
                  const void* Wp, int32_t Kp, int32_t Npad, int32_t Nreal,
                  const float* bias, const void* gate, int32_t gate_lowp, int64_t ldgate, int32_t relu,
                  int32_t accum, void* C, int64_t ldc, int32_t out_lowp, void* stream);
/* dW[N1, sum width_s] (+)= dY[M,N1]^T . [X_0 | X_1 | ...] and, if db != NULL, db[N1] (+)= colsum(dY)
 * (the bias gradient, produced by the same pass in bf16 mode).  Scratch: slab >= parts*N1*Ktot floats,
 * db_part >= max(parts, gn_colsum_blocks(M))*N1 floats, parts = gn_linear_wgrad_parts().
 * x_width: HOST int[nseg].  dY / X rows are fp32 or (dy_lowp / x_lowp, mode 1) bf16. */
int32_t gn_linear_wgrad_parts(int32_t mode, int32_t M, int32_t N1, int32_t nseg, const int32_t* x_width_host);
int gn_linear_wgrad(int32_t mode, const void* dY, int32_t dy_lowp, int64_t lddy, int32_t N1, int32_t nseg,
                    const void* const* x_ptr, int32_t x_lowp, const int64_t* x_ld, const int32_t* x_width,
                    int32_t M, float* slab, float* db_part, float* dW, float* db, int32_t accum, void* stream);

/* out[C] (+)= column sums of X[M, C]; part: >= gn_colsum_blocks(M)*C floats */
int32_t gn_colsum_blocks(int32_t M);
int gn_colsum(const float* X, int64_t ld, int32_t M, int32_t C, float* part, float* out, int32_t accum, void* stream);
int gn_reduce_slabs(const float* slab, int32_t nslab, int64_t count, float* out, int32_t accum, void* stream);

/* ---- fused EdgeConv (torch_geometric.nn.EdgeConv via DynEdgeConv, layers.py:55-60) ---- */

/* `saved`: opaque per-layer buffer of gn_edgeconv_saved_bytes() bytes holding the relu bits the
 * backward needs (layout: graphnet_amd/csrc/common.hpp saved_layout()). */
int64_t gn_edgeconv_saved_bytes(int32_t N, int32_t K, int32_t H1p, int32_t H2);
/* byte offsets of its three regions (HOST int64[3]: relu-bit words of the generic kernels, slot masks uint8 / uint16 [N][H2]
 * of the persistent kernels (S = 8 / 16 slots), h > 0 bits [N*S][H1p/8]) - for tests that read the arg slots of the max
 * variant back (the one-hot slot mask of (centre, column)) */
void gn_edgeconv_saved_offsets(int32_t N, int32_t K, int32_t H1p, int32_t H2, int64_t* offsets_host);

/* out[i, :H2] = sum_slots relu(relu(P[i]+Q[j]) . W2^T + b2); PQ: T[N, 2*H1p]; W2p: T[ceil128(H2)][H1p];
 * out: T[N, ldo].  coords (optional): fp32 [N][8], coords[i][d] = the fp32 value of output column
 * coord_cols_host[d], d < ncoord <= 8 — the coordinates DynEdgeConv re-runs k-NN on (layers.py:63-67),
 * kept in fp32 beside a bf16 `out`.  H1 <= H1p = real hidden width: columns H1..H1p-1 of P, Q and W2p are
 * zero padding (the packed layout), so the contraction may stop at H1.
 * Rounding in bf16 mode: out[i] is the fp32 slot sum rounded once (RNE); a centre with an overflow row gets a second
 * rounding, RNE(out[i] + m).  The two overflow paths differ there (gn_edgeconv_plan: ovf 1 / 2): the tiled overflow
 * kernels add the fp32 message m, the GEMM path adds the message it stored as bf16 - one rounding more in out[i], and
 * coords[i] (fp32 slot sum + m) then holds the bf16-rounded m, whereas it is the exact fp32 sum on the tiled path and for
 * every centre without an overflow row.  The backward differs likewise (dP[i] += the fp32 resp. the bf16 dpre row). */
int gn_edgeconv_fwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1,
                    const void* W2p, const float* b2, int32_t H2, void* out, int64_t ldo,
                    float* coords, const int32_t* coord_cols_host, int32_t ncoord,
                    void* saved, void* stream);
/* Which kernels the three passes of one layer run (host only, no launch): the answer of the one dispatch rule
 * (graphnet_amd/csrc/edge_plan.hpp) under this process's environment switches.  act: 0 = relu (the entries here), 1 = leaky
 * relu + max (gn_edgeconv_max_*), 2 = leaky relu + add (gn_edgeconv_leaky_*); has_ovf: the graph has an overflow list.
 * plan_host (HOST int32[8]) = { supported, persistent (table rows on the persistent bf16 kernels, else the tiled ones),
 * variant, ovf (0 no overflow list, 1 tiled overflow-row kernels, 2 overflow rows on the GEMM kernels), compact_shape
 * (gn_edgeconv_bwd_compact takes the layer), compact_model, shape_persistent, fwd_ws (the persistent forward is the
 * wave-specialised kernel, for `out` rows of pitch H2) }. */
void gn_edgeconv_plan(int32_t mode, int32_t K, int64_t N, int32_t H1p, int32_t H1, int32_t H2, int32_t act, int32_t has_ovf,
                      int32_t* plan_host);
/* dW2 / db2 partials: slab[nslab][H2][H1], db2_part[nslab][H2], nslab = gn_edgeconv_dw2_slabs();
 * reduce with gn_edgeconv_dw2_reduce (since ABI 6 NOT with gn_reduce_slabs: of the slabs reserved for overflow rows the
 * kernel writes only those whose row range holds overflow rows, and the reduction reads the count on the device).
 * Must run BEFORE gn_edgeconv_bwd of the same layer (it also records the first-relu bits that gn_edgeconv_bwd consumes). */
int32_t gn_edgeconv_dw2_slabs(int32_t mode, int32_t N, int32_t K, int32_t H1p, int32_t H2);
/* dW2 [H2][H1] and db2 [H2] (fp32) from the partials of gn_edgeconv_dw2 (leaky = 0) / gn_edgeconv_leaky_dw2 (leaky = 1)
 * called with the same mode, ovf_cnt, N, K, H1p, H1, H2: one launch, fixed summation order. */
int gn_edgeconv_dw2_reduce(int32_t mode, const int32_t* ovf_cnt, int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2,
                           int32_t leaky, const float* slab, const float* db2_part, float* dW2, float* db2, void* stream);
int gn_edgeconv_dw2(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1,
                    int32_t H2, const void* gout, int64_t ldg, void* saved,
                    float* slab, float* db2_part, void* stream);
/* gout: T[N, ldg]; dP: T[N, ldp] and dpre rows T[(N*S+N), H1p]; W2Tp: T[ceil128(H1p)][H2p] */
int gn_edgeconv_bwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                    const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H2,
                    const void* gout, int64_t ldg, const void* saved, const void* W2Tp, int32_t H2p,
                    void* dpre, void* dP, int64_t ldp, void* stream);
/* ---- compact dpre ----------------------------------------------------------------------------------------------
 * dpre (gn_edgeconv_bwd's edge-row output, read once by gn_edgeconv_dq_gather: the backward of PyG's scatter to x_j,
 * layers.py:60) is zero wherever the stored h-bits are clear - about half of it.  Compact variant, bit-identical
 * results: gn_edgeconv_dpre_plan (after gn_edgeconv_dw2, which writes the h-bits; before the backward) derives every
 * row's position from the h-bits; gn_edgeconv_bwd_compact writes the table rows WITHOUT their zero elements into
 * dpre_c (gn_edgeconv_dpre_compact_bytes() bytes, 16-byte aligned) and the overflow rows densely into
 * dpre_ovf[t][H1p] (T, t < *ovf_cnt <= N; may be NULL without an overflow list); gn_edgeconv_dq_gather_compact sums
 * them per source.  plan: gn_edgeconv_dpre_plan_bytes(N, K) bytes, 256-byte aligned, same buffer for the three calls.
 * Envelope (gn_edgeconv_dpre_compact_supported): bf16 mode, the persistent-kernel shapes with H1 <= 344. */
int32_t gn_edgeconv_dpre_compact_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H1, int32_t H2);
int64_t gn_edgeconv_dpre_plan_bytes(int32_t N, int32_t K);
int64_t gn_edgeconv_dpre_compact_bytes(int32_t N, int32_t K, int32_t H1p);
int gn_edgeconv_dpre_plan(int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2, const void* saved, void* plan, void* stream);
int gn_edgeconv_bwd_compact(const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src, const int32_t* ovf_cnt,
                            int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2, const void* gout, int64_t ldg,
                            const void* saved, const void* W2Tp, int32_t H2p, void* plan, void* dpre_c, void* dpre_ovf, void* dP,
                            int64_t ldp, void* stream);
int gn_edgeconv_dq_gather_compact(int32_t N, int32_t K, int32_t H1p, int32_t H1, int32_t H2, const void* saved, const void* plan,
                                  const void* dpre_c, const void* dpre_ovf, const int32_t* rev_ptr, const int32_t* rev_rows,
                                  const int32_t* hubs, const int32_t* nhubs, void* dQ, int64_t ldq, void* stream);

/* EdgeConvTito (models/components/layers.py:72-114: message nn([x_i, x_j - x_i, x_j]) with LeakyReLU after both Linear
 * layers, MAX aggregation; replaces PyG's EdgeConv.propagate + scatter-max and their backward) fused like the relu / add
 * variant above: out[i] = leaky(max_j (leaky(P[i] + Q[j]) W2^T + b2)), per (centre, column) the slot that supplied the
 * maximum is kept as a one-hot slot mask, and the backward kernels route the gradient to that edge row only.
 * bf16 mode, tables WITHOUT overflow rows (size K to the largest in-degree), K <= 16, H1p = H2 = 256 (the DynTrans
 * layer sizes of the reference: dynedge_kaggle_tito.py:44-47); gn_edgeconv_max_supported() says whether a shape is
 * inside that envelope - outside it the entry points return an error and the caller uses the unfused edge-row ops.
 * saved: gn_edgeconv_saved_bytes(N, K, H1p, H2) bytes; gout of gn_edgeconv_max_dw2 / _bwd must already hold
 * d(loss)/d(out) * leaky'(out) (gn_rownorm_act_bwd does that); slab: gn_edgeconv_max_dw2_slabs() * H2 * H1 floats,
 * db2_part: gn_edgeconv_max_dw2_slabs() * H2 floats (reduce with gn_reduce_slabs); dpre rows bf16[N*S, H1p]. */
int32_t gn_edgeconv_max_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H2);
int32_t gn_edgeconv_max_dw2_slabs(int32_t N, int32_t K, int32_t H1p);
int gn_edgeconv_max_fwd(const int32_t* nbr, int32_t N, int32_t K, const void* PQ, int32_t H1p, const void* W2p,
                        const float* b2, int32_t H2, void* out, int64_t ldo, void* saved, void* stream);
int gn_edgeconv_max_dw2(const int32_t* nbr, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                        const void* gout, int64_t ldg, void* saved, float* slab, float* db2_part, void* stream);
int gn_edgeconv_max_bwd(const int32_t* nbr, int32_t N, int32_t K, int32_t H1p, int32_t H2, const void* gout, int64_t ldg,
                        const void* saved, const void* W2Tp, int32_t H2p, void* dpre, void* dP, int64_t ldp, void* stream);

/* DynEdgeJINST's edge convolution (models/gnn/dynedge_jinst.py:56-98: DynEdgeConv(Sequential(Linear, LeakyReLU, Linear,
 * LeakyReLU), aggr="add"); replaces PyG's EdgeConv.propagate + scatter-add and their backward): the three entries above
 * with a leaky relu (torch's default slope 0.01) in place of BOTH relus - out[i] = sum_j leaky(leaky(P[i] + Q[j]) W2^T
 * + b2), saved bit = [pre-activation > 0].  Same arguments, workspaces (gn_edgeconv_saved_bytes, gn_edgeconv_dw2_slabs)
 * and call order (fwd ... dw2, then bwd) as gn_edgeconv_fwd / _dw2 / _bwd, both modes, overflow lists included; gout is
 * d(loss)/d(out) as it stands (the slopes are applied per edge row inside the kernels); _bwd also takes the real hidden
 * width H1 (all three calls of a layer must pass the same one).  In bf16 mode the persistent kernels run for the
 * DynEdge layer shapes with H1 <= 336 (gn_edgeconv_leaky_supported()): their forward leaves one 64-bit row-validity
 * word per 64-row tile in `saved` - with a leaky second activation an EXISTING row whose bit is clear still passes 0.01
 * of the gradient, a slot without an edge nothing.  Other shapes run on the tiled kernels. */
int32_t gn_edgeconv_leaky_supported(int32_t mode, int32_t K, int32_t H1p, int32_t H1, int32_t H2);
int gn_edgeconv_leaky_fwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, const void* W2p,
                          const float* b2, int32_t H2, void* out, int64_t ldo, float* coords, const int32_t* coord_cols_host,
                          int32_t ncoord, void* saved, void* stream);
int gn_edgeconv_leaky_dw2(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                          const void* gout, int64_t ldg, void* saved, float* slab, float* db2_part, void* stream);
int gn_edgeconv_leaky_bwd(int32_t mode, const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src,
                          const int32_t* ovf_cnt, int32_t N, int32_t K, const void* PQ, int32_t H1p, int32_t H1, int32_t H2,
                          const void* gout, int64_t ldg, const void* saved, const void* W2Tp, int32_t H2p, void* dpre,
                          void* dP, int64_t ldp, void* stream);

/* dQ[j] (T[N, ldq]) = sum of dpre rows that gathered from j (ascending row id, fp32 accumulation).
 * hubs / nhubs (optional, may be NULL): what gn_rev_build leaves in its `cursor` / `tmp[0]` workspace - the
 * nodes with 65..16384 in-edges (sorted lists); they are then summed by a 16-wave workgroup each, in a
 * fixed block order, instead of by one wave. */
int gn_edgeconv_dq_gather(int32_t mode, const void* dpre, int32_t H1p, const int32_t* rev_ptr,
                          const int32_t* rev_rows, const int32_t* hubs, const int32_t* nhubs, int32_t N,
                          void* dQ, int64_t ldq, void* stream);

/* ---- unfused edge-MLP building blocks: DynEdge(activation_layer="gelu" / add_norm_layer=True) ----------
 * (dynedge.py:160-167,198-231: GELU and LayerNorm after every Linear of the edge and post MLPs.)  The fused
 * kernels above keep one relu bit per activation; GELU / LayerNorm need the pre-activations and a reduction
 * over the whole row, so these variants run on edge-row tensors [N*S + N, .] in HBM, fp32. */
/* ic[r], jc[r] = centre / source of edge row r (jc = -1: empty slot), r < N*S + N */
int gn_edge_rows(const int32_t* nbr, const int32_t* ovf_centre, const int32_t* ovf_src, const int32_t* ovf_cnt,
                 int32_t N, int32_t K, int32_t* ic, int32_t* jc, void* stream);
/* The same (ic, jc) for the EXISTING edges only (with k = 9 a centre has 16 slots: 17 N rows of which ~9 N exist): centre
 * i's rows are row_ptr[i] .. row_ptr[i+1] (its table slots in slot order, then its overflow edge), row_ptr[N] = their number;
 * ic / jc have N*K + N entries, (0, -1) beyond row_ptr[N].  ovf: the per-centre array gn_knn_graph wrote (or NULL);
 * deg: N ints, tmp: gn_scan_tmp_ints(N) ints of scratch.  gn_segment_rows_sum: out[i] = sum of centre i's rows (the sum
 * gn_slot_sum forms, same order); gn_rev_rows_compact: the reverse lists of gn_rev_build* in compact row ids. */
int gn_rows_compact(const int32_t* nbr, const int32_t* ovf, int32_t N, int32_t K, int32_t* deg, int32_t* tmp, int32_t* row_ptr,
                    int32_t* ic, int32_t* jc, void* stream);
int gn_segment_rows_sum(const float* m, int64_t ldm, int32_t C, int32_t N, const int32_t* row_ptr, float* out, int64_t ldo,
                        int32_t m_lowp /* m holds bf16 */, void* stream);
int gn_rev_rows_compact(const int32_t* nbr, const int32_t* ovf_centre, int32_t N, int32_t K, const int32_t* row_ptr,
                        const int32_t* rev_ptr, const int32_t* rev_rows, int32_t* out, void* stream);
/* pre[r, :H1p] = act(P[ic[r]] + Q[jc[r]]) (PQ fp32 [N, 2*H1p]), 0 for empty slots; act 3 (identity: the
 * pre-activation) or 2 (leaky relu applied at once; its derivative is recovered from the result's sign);
 * pre fp32, or bf16 when pre_lowp */
int gn_edge_gather_pre(const float* PQ, int32_t H1p, const int32_t* ic, const int32_t* jc, int64_t rows, int32_t act,
                       void* pre, int32_t pre_lowp, void* stream);
/* a[r, c] = act(gamma ? LayerNorm(z[r, :C]) : z[r, c]); 0 for C <= c < Cpad and for rows with valid[r] < 0;
 * act: 0 relu, 1 gelu (erf), 2 leaky relu (0.01), 3 identity; stats[r] = (mean, rstd) when gamma != NULL; Cpad <= 512.
 * The result goes to a (fp32) and / or a_bf16 (the copy the MFMA GEMMs consume; either may be NULL, not both). */
int gn_rownorm_act_fwd(const float* z, int64_t ldz, int32_t C, const int32_t* valid, const float* gamma,
                       const float* beta, float eps, int32_t act, float* a, int64_t lda, int32_t Cpad,
                       float* stats, int64_t rows, void* a_bf16, int64_t lda_bf16, int32_t z_lowp, void* stream);
/* (z_lowp: z holds bf16 values - a pre-activation kept in bf16; ldz in elements.) */
/* dz = d(loss)/dz given g = d(loss)/da (row gidx ? gidx[r] : r of g); with LayerNorm also partial column sums
 * t_dy[nblk, C], t_dyx[nblk, C], nblk = gn_rownorm_bwd_blocks(rows) (one row per workgroup), whose column
 * sums (gn_colsum over nblk rows) are dbeta and dgamma.  (Up to ABI 5 these were per-row terms [rows, C].) */
int32_t gn_rownorm_bwd_blocks(int64_t rows);
int gn_rownorm_act_bwd(const float* g, int64_t ldg, const int32_t* gidx, const float* z, int64_t ldz, int32_t C,
                       const int32_t* valid, const float* gamma, const float* beta, const float* stats,
                       int32_t act, float* dz, int64_t lddz, int32_t Cpad, float* t_dy, float* t_dyx,
                       int64_t rows, void* dz_bf16, int64_t lddz_bf16, const int32_t* argrow, int32_t z_lowp,
                       void* stream);
/* (dz fp32 and / or dz_bf16, as above.  argrow != NULL (needs gidx): the rows fed a max aggregation
 * (gn_slot_reduce) - g[gidx[r], c] reaches row r only where argrow[gidx[r]*C + c] == r.  z_lowp: bit 0 - z holds bf16,
 * bit 1 - g holds bf16.) */
/* out[i, :C] = sum over the slots (and the overflow row) of centre i of m[row, :C] */
int gn_slot_sum(const float* m, int64_t ldm, int32_t C, const int32_t* nbr, const int32_t* ovf_centre,
                const int32_t* ovf_src, const int32_t* ovf_cnt, int32_t N, int32_t K, float* out, int64_t ldo,
                void* stream);

/* EdgeConv aggregation over a centre's edge rows (torch_geometric MessagePassing aggr; DynEdgeConv default "max",
 * layers.py:20-50): aggr 0 add, 1 mean, 2 max (first occurrence, centres without edges -> 0).  jc from
 * gn_edge_rows.  Outputs besides out[N, ldo]: ovf_row[N] (overflow row of a centre or -1), deg[N] (edges per
 * centre), argrow[N*C] (aggr = max only).  gn_slot_reduce_bwd expands gout[N, ldg] to the edge rows. */
int gn_slot_reduce(const float* m, int64_t ldm, int32_t C, const int32_t* nbr, const int32_t* ovf_centre,
                   const int32_t* ovf_src, const int32_t* ovf_cnt, int32_t N, int32_t K, const int32_t* jc,
                   int32_t aggr, float* out, int64_t ldo, int32_t* ovf_row, int32_t* deg, int32_t* argrow,
                   int32_t post_act, void* stream);
/* (post_act 3: none; 2: leaky relu applied to the max - a strictly increasing activation commutes with max, so
 * the N*S edge rows need not be activated first) */
int gn_slot_reduce_bwd(const float* gout, int64_t ldg, int32_t C, const int32_t* ic, const int32_t* jc,
                       int64_t rows, int32_t aggr, const int32_t* deg, const int32_t* argrow, float* grows,
                       int64_t ldr, int32_t Cpad, void* stream);

/* ---- BatchNorm1d inside an EdgeConv MLP (ParticleNeT, models/gnn/particlenet.py:172-198) ---- */
/* torch.nn.BatchNorm1d over the edges of the batch = the rows r with valid[r] >= 0 of an edge-row tensor.
 * Training forward: gn_bn_sums(mode 0) -> sums[2C] = (sum z, sum z^2); gn_bn_finalize -> mean, rstd (biased
 * variance + eps), var_unbiased (for running_var); gn_bn_act_fwd -> a = act((z - mean) rstd gamma + beta) (fp32 or
 * bf16, 0 on empty rows).  Eval: gn_bn_act_fwd with the running statistics.  Backward: gn_bn_sums(mode 1, g = dL/da)
 * -> sums = (dbeta, dgamma); gn_bn_act_bwd -> dz (sums = NULL: eval-mode backward).  n_valid: DEVICE int[1], number
 * of valid rows.  part: gn_bn_blocks(rows) * 2C floats of scratch.  Fixed-order reductions, no atomics. */
int64_t gn_bn_blocks(int64_t rows);
int gn_bn_sums(int32_t mode, int32_t act, const float* z, int64_t ldz, int64_t rows, int32_t C, const int32_t* valid,
               const float* g, int64_t ldg, const float* mean, const float* rstd, const float* gamma, const float* beta,
               float* part, float* sums, void* stream);
int gn_bn_finalize(const float* sums, const int32_t* n_valid, int32_t C, float eps, float* mean, float* rstd,
                   float* var_unbiased, void* stream);
int gn_bn_act_fwd(const float* z, int64_t ldz, int64_t rows, int32_t C, const int32_t* valid, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, int32_t act, void* a, int64_t lda,
                  int32_t Cpad, int32_t a_lowp, void* stream);
int gn_bn_act_bwd(const float* g, int64_t ldg, const float* z, int64_t ldz, int64_t rows, int32_t C,
                  const int32_t* valid, const float* mean, const float* rstd, const float* gamma, const float* beta,
                  const float* sums, const int32_t* n_valid, int32_t act, void* dz, int64_t lddz, int32_t Cpad,
                  int32_t dz_lowp, void* stream);

/* ---- operand copies of the weights ------------------------------------------------------- */
/* One launch rewrites every padded / transposed / bf16 copy of the weights the kernels above consume
 * (what torch.nn.Linear does implicitly with its own weight).  desc: DEVICE int64[ndesc][10] =
 * {src, src2 (or 0), dst, s_row, s_col, d_pitch, rows, cols, dst_is_bf16, 0}:
 * dst[r*d_pitch + c] = src[r*s_row + c*s_col] - (src2 ? src2[r*s_row + c*s_col] : 0), strides in elements. */
int gn_pack_weights(const int64_t* desc, int32_t ndesc, void* stream);

/* ---- pooling (torch_scatter.scatter_{min,max,sum,mean}, dynedge.py:251-264) ------------ */
/* codes: HOST int[ns], 0 = min, 1 = max, 2 = sum, 3 = mean; out[B, ns*C] */
int gn_segment_pool_fwd(const float* x, int64_t ldx, int32_t C, const int32_t* ptr, int32_t B,
                        const int32_t* codes_host, int32_t ns, float* out, int32_t* argmin, int32_t* argmax,
                        void* stream);
int gn_segment_pool_fwd_ws(const float* x, int64_t ldx, int32_t C, const int32_t* ptr, int32_t B, int32_t N, const int32_t* codes_host,
                           int32_t ns, float* out, int32_t* argmin, int32_t* argmax, void* scratch, void* stream);
int gn_segment_pool_bwd(const float* gout, int32_t C, const int32_t* ptr, const int32_t* batch, int32_t N,
                        const int32_t* codes_host, int32_t ns, const int32_t* argmin, const int32_t* argmax,
                        const float* gate, int64_t ldgate, void* dx, int64_t lddx, int32_t dx_lowp, void* stream);
/* (dx: fp32, or bf16 when dx_lowp) */

/* ---- ragged attention with the spacetime bias of DeepIce (models/components/layers.py:389-499, embedding.py:139-175) ---- */
/* Attention_rel without the [B, L, L, dh] bias tensor.  With s_ij the sinusoidal embedding (width DH) of the clipped
 * 4-distance of pulses i, j of one event and R_ij = W s_ij + b its projection, the reference's scores and outputs are
 *   q~_ih . k_jh + q~_ih . R_ij = q~_ih . k_jh + (W^T q~_ih) . s_ij + const_j,   sum_j a_ihj (v_jh + R_ij) = O_ih + W U_ih + b,
 * q~ = q / sqrt(DH), U_ih = sum_j a_ihj s_ij.  These entries take qkv[N, ld] = [Q | K | V] (each H*DH wide), the per-row
 * operand qp[N, ldqp] = W^T q~ per head (H*DH wide; the 1/sqrt(DH) is ALREADY in it), xt[N, ldxt] (columns 0-2 position,
 * column 3 time, ldxt >= 4) and freq[DH/2] (the frequencies of SinusoidalPosEmb(DH), formed on the host), recompute s_ij
 * per pair and return out = O, u = U (both [N, H*DH]) and lse2[N, H] = log2 of the softmax denominators.  W and b are
 * applied by the caller.  All tensors fp32; DH = 32 (gn_rel_attention_supported); ptr / tile_ptr as gn_attention_fwd
 * (the plan of gn_attention_plan); row pitches multiples of 4 floats.  No atomics: two runs agree bit for bit.
 * CONTRACT of the pair argument, fp32, every operation rounded on its own (no fused multiply-add), differences query - key:
 *   ds = ((dx*dx + dy*dy) + dz*dz) - (dt*18)*(dt*18),  d = sign(ds) * sqrt(|ds|),  a = 1024 * min(max(d, -4), 4),
 *   s_ij = [sin(a * freq[k]) | cos(a * freq[k])], k < DH/2, the products a * freq[k] and the sines to ~1e-6 absolute.
 * gn_rel_attention_bwd: given dout, du (gradients w.r.t. out, u) and the forward's out, u, lse2 -> dqkv[N, lddq]
 * (3*H*DH wide) and dqp[N, lddqp]; xt and freq get no gradient; delta[N, H] fp32 is scratch. */
int gn_rel_attention_supported(int32_t DH);
int gn_rel_attention_fwd(const float* qkv, int64_t ld, const float* qp, int64_t ldqp, const float* xt, int64_t ldxt,
                         const float* freq, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr, int32_t B,
                         int32_t N, float* out, int64_t ldo, float* u, int64_t ldu, float* lse2, void* stream);
int gn_rel_attention_bwd(const float* qkv, int64_t ld, const float* qp, int64_t ldqp, const float* xt, int64_t ldxt,
                         const float* freq, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr, int32_t B,
                         int32_t N, const float* out, int64_t ldo, const float* u, int64_t ldu, const float* dout,
                         int64_t lddo, const float* du, int64_t lddu, const float* lse2, float* delta, float* dqkv,
                         int64_t lddq, float* dqp, int64_t lddqp, void* stream);

/* ---- ragged multi-head self attention (DynTrans, models/components/layers.py:166-197) ---- */
/* Replaces to_dense_batch + torch.nn.TransformerEncoder's attention + x[mask]: every pulse attends to the
 * pulses of its own event (ptr), nothing is padded.  qkv[N, ld] = [Q | K | V], each H*DH wide (the in_proj
 * output); tile_ptr = the plan of gn_attention_plan (int32[2B+1]: first 64-row tile of every event in plan order,
 * then the event at each position; sorted != 0: largest events first, so that the launch does not end on the tail
 * of the longest event); out[N, ldo] = softmax(Q K^T / sqrt(DH)) V per head, heads side by side;
 * lse2[N, H] fp32 = log2 of the softmax denominators (saved for the backward).  gn_attention_bwd: dqkv[N, lddq] =
 * gradient w.r.t. qkv given dout; delta[N, H] fp32 is scratch.
 * lowp = 0: qkv / out / dout / dqkv are fp32, exact-fp32 kernels on the vector ALU, DH in {8, 16, 32, 64}.
 * lowp = 1: those four tensors are bf16, products on the matrix core (fp32 softmax statistics and accumulation),
 *           DH in {32, 64}.
 * drop_thresh != 0: dropout on the attention probabilities (see gn_dropout for the rule). */
int gn_attention_plan(const int32_t* ptr, int32_t B, int32_t* plan, int32_t sorted, void* stream);
int gn_attention_fwd(int32_t lowp, const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr,
                     const int32_t* tile_ptr, int32_t B, int32_t N, void* out, int64_t ldo, float* lse2, uint32_t drop_seed,
                     uint32_t drop_thresh, void* stream);
int gn_attention_bwd(int32_t lowp, const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr,
                     const int32_t* tile_ptr, int32_t B, int32_t N, const void* out, int64_t ldo, const void* dout,
                     int64_t lddo, const float* lse2, float* delta, void* dqkv, int64_t lddq, uint32_t drop_seed,
                     uint32_t drop_thresh, void* stream);

/* The same with the dropout decisions SAVED (bf16 tensors, matrix-core kernels only; ABI 4): the forward evaluates the
 * keep rule and also stores every decision as a bit, once per orientation, the backward reads the bits instead of
 * re-evaluating the hash twice per probability.  An event of n pulses has W = ceil(n / 32) blocks per side and W * W
 * tiles of 32 words; evoff[B + 1] (int64, device) = running sum of W * W over the events in ptr order;
 * plane_words = 32 * evoff[B]; bits_r / bits_c: uint32[H * plane_words] each:
 *   bits_r: tile (query block qb, key block kb) at evoff[e] + qb * W + kb, word c = the 32 key bits of query 32 qb + c
 *   bits_c: tile (key block kb, query block qb) at evoff[e] + kb * W + qb, word c = the 32 query bits of key 32 kb + c
 * Same results as gn_attention_fwd / gn_attention_bwd with the same seed and threshold, bit for bit. */
int gn_attention_fwd_bits(const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr,
                          int32_t B, int32_t N, void* out, int64_t ldo, float* lse2, uint32_t drop_seed, uint32_t drop_thresh,
                          uint32_t* bits_r, uint32_t* bits_c, const int64_t* evoff, int64_t plane_words, void* stream);
int gn_attention_bwd_bits(const void* qkv, int64_t ld, int32_t H, int32_t DH, const int32_t* ptr, const int32_t* tile_ptr,
                          int32_t B, int32_t N, const void* out, int64_t ldo, const void* dout, int64_t lddo, const float* lse2,
                          float* delta, void* dqkv, int64_t lddq, uint32_t drop_thresh, const uint32_t* bits_r,
                          const uint32_t* bits_c, const int64_t* evoff, int64_t plane_words, void* stream);

/* ---- dropout (torch.nn.Dropout inside TransformerEncoderLayer / MultiheadAttention, layers.py:149-160) ---- */
/* Counter-based: element (r, c) of stream `seed` is kept iff mix32(mix32(seed ^ r*0x9E3779B1) ^ c*0x85EBCA77) >=
 * thresh, thresh = round(p * 2^32), kept values are scaled by 1 / (1 - thresh / 2^32); nothing is stored, the
 * backward recomputes the decisions from the same seed (apply gn_dropout to the gradient).  thresh = 0 disables.
 * y[r, c] = (res ? res[r, c] : 0) + dropout(x)[r, c]; x / y fp32 or bf16 (in place allowed), res fp32.
 * The attention kernels drop the softmax probabilities with ONE hash per (query row q, pair of keys, head): keys 2m and
 * 2m + 1 of an event (indices inside the event) take the low / high halfword of
 * mix32(mix32(seed ^ q*0x9E3779B1) ^ (m*H + head)*0x85EBCA77), kept iff the halfword >= thresh >> 16. */
int gn_dropout(const void* x, int64_t ldx, int32_t x_lowp, const float* res, int64_t ldres, void* y, int64_t ldy,
               int32_t y_lowp, int64_t rows, int32_t cols, uint32_t seed, uint32_t thresh, void* stream);

/* ---- the whole backbone pass behind ONE entry -------------------------------------------------------------------
 * DynEdge.forward (models/gnn/dynedge.py:295-349) from the standardised pulses to the pooled features - layer-1 k-NN
 * graph (unless the caller brings one), global variables + broadcast, nconv x [P|Q GEMM, fused EdgeConv, k-NN
 * re-clustering on `knn_cols` of the new features (models/components/layers.py:55-69)], post-processing MLP on the
 * skip-cat, global pooling - and its backward, each enqueued by one call: the same kernels with the same arguments in
 * the same order as the per-op entry points above (results are bit-identical), without ~110 host crossings per pass.
 * The read-out MLP, task head and loss stay with the caller (models/standard_model.py:71-119).
 * Envelope: two-layer relu edge MLPs (the fused path), >= 1 pooling scheme, <= 5 conv layers; anything else runs on
 * the per-op entry points.  All pointers inside the descriptor are DEVICE pointers except the int arrays of the
 * descriptor itself.  Parameters: fp32, torch.nn.Linear layout ([out, in], contiguous): W1[l] [H1, 2 Fin_l] =
 * [Wa | Wb], W2[l] [H2, H1], Wp[t] [P_t, in_t] with in_0 = F + G + sum H2.
 * Workspaces (caller-owned, 256-byte aligned): wws - gn_dynedge_wws_bytes(), PERSISTENT across steps and zeroed once by
 * the caller (operand copies of the weights; pads stay zero); ws - gn_dynedge_ws_bytes(), per step, written by the
 * forward and read by the backward of the same step; bws - gn_dynedge_bwd_ws_bytes(), backward scratch. */
#define GN_DYNEDGE_MAX_CONV 5
#define GN_DYNEDGE_MAX_POST 4
typedef struct GnDynEdgeDesc {
    int32_t struct_bytes;                 /* sizeof(GnDynEdgeDesc) */
    int32_t mode;                         /* GN_MODE_F32 / GN_MODE_BF16 */
    int32_t N, B, F;                      /* pulses, events, input features */
    int32_t G;                            /* global variables broadcast to the pulses before layer 1: F + 5, or 0 */
    int32_t k, strict;                    /* nb_neighbours; 0 = knn_graph semantics (k+1 with self, then mask) */
    int32_t n_graph_cols, graph_cols[8];  /* columns of x the layer-1 graph is built on (ignored with nbr0) */
    int32_t n_knn_cols, knn_cols[8];      /* features_subset: columns of a conv output the next graph is built on */
    int32_t nconv, H1[GN_DYNEDGE_MAX_CONV], H2[GN_DYNEDGE_MAX_CONV];
    int32_t npost, P[GN_DYNEDGE_MAX_POST];
    int32_t npool, pool_codes[4];         /* 0 min, 1 max, 2 sum, 3 mean */
    int32_t K0, event_local0;             /* caller-built layer-1 table: its K; 1 = no edge leaves its event */
    const float* x; int64_t ldx;          /* [N, ldx] standardised pulses */
    const int32_t* ptr; const int32_t* batch; const int32_t* n_pulses;
    const int32_t* nbr0; const int32_t* ovf0; const int32_t* ovf0_pos; const int32_t* ovf0_centre;
    const int32_t* ovf0_src; const int32_t* ovf0_cnt;      /* optional caller-built layer-1 table (gn_edge_index_to_table) */
    const float* W1[GN_DYNEDGE_MAX_CONV]; const float* b1[GN_DYNEDGE_MAX_CONV];
    const float* W2[GN_DYNEDGE_MAX_CONV]; const float* b2[GN_DYNEDGE_MAX_CONV];
    const float* Wp[GN_DYNEDGE_MAX_POST]; const float* bp[GN_DYNEDGE_MAX_POST];
    void* wws; int64_t wws_bytes;
    void* ws; int64_t ws_bytes;
    void* stream;
} GnDynEdgeDesc;
typedef struct GnDynEdgeGrads {           /* outputs of the backward: fp32, same shapes as the parameters */
    float* dW1[GN_DYNEDGE_MAX_CONV]; float* db1[GN_DYNEDGE_MAX_CONV];
    float* dW2[GN_DYNEDGE_MAX_CONV]; float* db2[GN_DYNEDGE_MAX_CONV];
    float* dWp[GN_DYNEDGE_MAX_POST]; float* dbp[GN_DYNEDGE_MAX_POST];
} GnDynEdgeGrads;
int64_t gn_dynedge_wws_bytes(const GnDynEdgeDesc* d);        /* -1: descriptor outside the envelope */
int64_t gn_dynedge_ws_bytes(const GnDynEdgeDesc* d);
int64_t gn_dynedge_bwd_ws_bytes(const GnDynEdgeDesc* d);
/* global_vars: fp32 [B, F + 5] (dynedge.py:266-293); pooled: fp32 [B, npool * P_last] (dynedge.py:251-264) */
int gn_dynedge_fwd(const GnDynEdgeDesc* d, float* global_vars, float* pooled);
/* grad_pooled: fp32 [B, npool * P_last]; the descriptor (incl. ws) must be the forward's */
int gn_dynedge_bwd(const GnDynEdgeDesc* d, const float* grad_pooled, void* bws, int64_t bws_bytes, const GnDynEdgeGrads* grads);
const char* gn_step_last_error(void);
/* HIP events around every op group inside the two entries (bench.py's live kernel durations).  enable(1), run steps,
 * gn_step_timers_read -> text lines "name launches total_ms" (synchronises the device; returns the bytes needed). */
void gn_step_timers_enable(int32_t on);
int64_t gn_step_timers_read(char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHNET_AMD_H */
