// graphnet_amd/csrc/launchers.hpp — host launcher prototypes shared with the C ABI (cabi.hip).
#pragma once
#include "common.hpp"

namespace gn {
// graph.hip
hipError_t launch_knn_plan(const int* ptr, int B, int* tile_ptr, hipStream_t st);
hipError_t launch_knn(const float* x, long long ldx, const int* cols, int D, const int* ptr, const int* tile_ptr,
                      int B, int N, int k, int strict, int* nbr, int* ovf, void* ws, hipStream_t st);
long long knn_ws_bytes(int B, int N, int D);
hipError_t launch_minkowski_knn(const float* x, long long ldx, const int* space_cols, int DS, int time_col, float c,
                                float time_like_weight, const int* ptr, const int* tile_ptr, int B, int N, int k, int* nbr,
                                hipStream_t st);
hipError_t launch_radius_graph(const float* x, long long ldx, const int* cols, int D, float r, const int* ptr,
                               const int* tile_ptr, int B, int N, int cap, int* nbr, int* deg, int* work, hipStream_t st);
long long radius_work_ints(int B, int N);
hipError_t launch_scan(const int* in, int* out, int n, int* tmp, int* total, hipStream_t st);
hipError_t launch_ovf_compact(const int* ovf, int N, int* flag_pos, int* tmp, int* ovf_centre, int* ovf_src,
                              int* ovf_cnt, hipStream_t st);
int rev_event_slices(int B);
hipError_t launch_rev_build_events(const int* nbr, int N, int K, int S, const int* ovf, const int* ovf_pos, const int* ptr,
                                   int B, int* rev_ptr, int* rev_rows, int* ev, int* scratch, int* hubs, int* nhubs,
                                   int* tmp, int* pairs, hipStream_t st);
long long rev_pairs_ints(int B, int N, int K);
hipError_t launch_rev_build(const int* nbr, int N, int K, int S, const int* ovf_src, const int* ovf_cnt,
                            int* rev_ptr, int* cursor, int* tmp, int* rev_rows, hipStream_t st);
hipError_t launch_table_degree(const int* nbr, const int* ovf, int N, int K, int* deg, hipStream_t st);
hipError_t launch_table_to_edges(const int* nbr, const int* ovf, int N, int K, const int* off, long long E,
                                 long long* edge_index, hipStream_t st);
hipError_t launch_edges_to_table(const long long* edge_index, long long E, int N, int K, int* first, int* nbr,
                                 int* ovf, int* err, hipStream_t st);
// scratch (optional, globals_scratch_bytes(B, N)) and N: a batch of a few huge events runs one workgroup per event SLICE (same result)
long long globals_scratch_bytes(int B, int N);
hipError_t launch_globals(const float* x, long long ldx, int F, const int* ptr, int B, const int* nbr, const int* ovf,
                          int K, const int* n_pulses, float* out, hipStream_t st, void* scratch = nullptr, int N = 0);
hipError_t launch_concat_globals(const float* x, long long ldx, int F, const float* gv, int G, const int* batch, int N,
                                 void* x0, int ld0, int out_lowp, hipStream_t st);
hipError_t launch_ptr_to_batch(const int* ptr, int B, int* batch, hipStream_t st);
hipError_t launch_standardize(float* x, long long ldx, int N, int F, const int* nops, const int* op, const float* c,
                              hipStream_t st);
// nodes.hip
int percentile_lds_max();
long long percentile_work_ints(int B, int N);
hipError_t launch_percentile_clusters(const float* x, long long ldx, int N, const int* ptr, int B, const int* cluster_cols, int C,
                                      const int* summ_cols, int S, const double* q, int P, int add_counts, float* out,
                                      long long ldo, int* out_ptr, int* work, hipStream_t st);
long long dom_time_series_work_ints(int B, int N);
hipError_t launch_dom_time_series(const float* x, long long ldx, int F, int N, const int* ptr, int B, const int* id_cols, int C,
                                  int time_col, int charge_col, float* out, long long ldo, int* series_ptr, int* dom_ptr,
                                  int* work, hipStream_t st);
hipError_t launch_icemix_nodes(const float* x, long long ldx, int F, int N, const int* ptr, int B, int L, int hlc_col, int z_col,
                               const double* table, int T, unsigned int seed, const unsigned int* event_ids, int key_bits,
                               float* out, long long ldo, int* out_ptr, int* ids, hipStream_t st);
// rnn.hip
int gru_supported(int I, int H);
long long gru_saved_floats(int T, int H);
long long gru_bwd_work_floats(int T, int I, int H);
hipError_t launch_gru_series_fwd(const float* xs, long long ldx, int T, int I, const int* series_ptr, int M, int H,
                                 const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* out,
                                 float* saved, hipStream_t st);
hipError_t launch_gru_series_bwd(const float* dout, const float* saved, const float* xs, long long ldx, int T, int I,
                                 const int* series_ptr, int M, int H, const float* w_hh, float* dw_ih, float* db_ih,
                                 float* dw_hh, float* db_hh, float* work, hipStream_t st);
hipError_t launch_dom_series_summary(const float* x, long long ldx, int F, int N, const int* series_ptr, int M, int charge_col,
                                     float* out, long long ldo, hipStream_t st);
// gemm.hip
hipError_t launch_gemm_nt(int mode, const Segs& a, int a_lowp, int M, const void* Wp, int Kp, int Npad, int Nreal,
                          const Epi& epi, void* C, long long ldc, int out_lowp, hipStream_t st);
int gemm_tn_parts(int mode, int M, int N1, const int* widths, int nseg);
hipError_t launch_gemm_tn(int mode, const void* dY, int dy_lowp, long long lddy, int N1, const Segs& x, int x_lowp,
                          int M, float* slab, float* db_part, float* dW, float* db, int accum, hipStream_t st);
hipError_t launch_gemm_tn_parts_only(const void* dY, long long lddy, int N1, const void* X, long long ldx, int K, int M,
                                     const int* m_dev, float* slab, float* db_part, hipStream_t st);
int colsum_blocks(int M);
hipError_t launch_colsum(const float* X, long long ld, int M, int C, float* part, float* out, int accum, hipStream_t st);
hipError_t launch_reduce_slabs(const float* slab, int nslab, long long count, float* out, int accum, hipStream_t st);
hipError_t launch_reduce_slabs2(const float* slab0, long long count0, float* out0, const float* slab1, long long count1, float* out1,
                                int nmain, int novf, const int* ovf_cnt, int ovf_rps, hipStream_t st);
// edgeconv.hip
int edge_slots(int K);
long long edge_dw2_splits(long long rows);
hipError_t launch_edge_fwd(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H1, const void* W2p, const float* b2,
                           int H2, void* out, long long ldo, float* coords, const int* coord_cols, int ncoord,
                           void* saved, hipStream_t st, int act = 0);
// act (all passes of a layer take the same, see edge_plan.hpp): 0 = relu, 1 = leaky relu + max aggregation (EdgeConvTito:
// fused kernels or hipErrorNotSupported, edge_max_supported()), 2 = leaky relu after both layers (DynEdgeJINST);
// H1 (real hidden width) is needed with act = 2
hipError_t launch_edge_bwd(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H2, const void* gout,
                           long long ldg, const void* saved, const void* W2Tp, int H2p, void* dpre,
                           void* dP, long long ldp, hipStream_t st, int act = 0, int H1 = 0);
int edge_leaky_supported(int mode, int K, int H1p, int H1, int H2);
// out[8]: the EdgePlan fields in declaration order, then whether the persistent forward is wave-specialised (host only)
void edge_plan_query(int mode, int K, long long N, int H1p, int H1, int H2, int act, bool has_ovf, int* out);
int edge_dw2_slabs(int mode, int N, int K, int H1p, int H2);
hipError_t launch_edge_dw2(int mode, const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout,
                           long long ldg, void* saved, float* slab, float* db2_part, hipStream_t st, int act = 0);
// dW2 [H2][H1] and db2 [H2] from the partials launch_edge_dw2 (same mode / shape / act) left in slab and db2_part
hipError_t launch_edge_dw2_reduce(int mode, const EdgeGraph& g, int H1p, int H1, int H2, const float* slab, const float* db2_part,
                                  float* dW2, float* db2, hipStream_t st, int act = 0);
int edge_max_supported(int mode, int K, int H1p, int H2);
int edge_max_dw2_slabs(int N, int K, int H1p);
hipError_t launch_dq_gather(int mode, const void* dpre, int H1p, const int* rev_ptr, const int* rev_rows,
                            const int* hubs, const int* nhubs, int N, void* dQ, long long ldq, hipStream_t st);
// compact dpre (dpre_compact.hip + edgeconv.hip): plan workspace of dpre_plan_layout(N, K, nullptr).total bytes
struct DprePlan { unsigned short* rowoff; int* tilesize16; int* tilebase; int* tmp; long long total; };
DprePlan dpre_plan_layout(int N, int K, void* base);
int dpre_compact_supported(int mode, int K, int H1p, int H1, int H2);
long long dpre_compact_bytes(int N, int K, int H1p);
hipError_t launch_dpre_plan_saved(int N, int K, int H1p, int H1, int H2, const void* saved, void* plan, hipStream_t st);
hipError_t launch_edge_bwd_cp(const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout, long long ldg,
                              const void* saved, const void* W2Tp, int H2p, void* plan, void* dpre_c, void* dpre_ovf, void* dP,
                              long long ldp, hipStream_t st);
hipError_t launch_dq_gather_cp_saved(int N, int K, int H1p, int H1, int H2, const void* saved, const void* plan, const void* dpre_c,
                                     const void* dpre_ovf, const int* rev_ptr, const int* rev_rows, const int* hubs,
                                     const int* nhubs, void* dQ, long long ldq, hipStream_t st);
// generic.hip
hipError_t launch_edge_rows(const EdgeGraph& g, int S, int* ic, int* jc, hipStream_t st);
hipError_t launch_rows_compact(const EdgeGraph& g, const int* ovf, int* deg, int* tmp, int* row_ptr, int* ic, int* jc, hipStream_t st);
hipError_t launch_segment_rows_sum(const float* m, long long ldm, int C, int N, const int* row_ptr, float* out, long long ldo,
                                   int m_lowp, hipStream_t st);
hipError_t launch_rev_rows_compact(const EdgeGraph& g, int S, const int* row_ptr, const int* rev_ptr, const int* rev_rows, int* out,
                                   hipStream_t st);
hipError_t launch_edge_gather_pre(const float* PQ, int H1p, const int* ic, const int* jc, long long rows, int act,
                                  void* pre, int pre_lowp, hipStream_t st);
hipError_t launch_rownorm_act_fwd(const float* z, long long ldz, int C, const int* valid, const float* gamma,
                                  const float* beta, float eps, int act, float* a, long long lda, int Cpad, float* stats,
                                  long long rows, void* a16, long long lda16, int z_lowp, hipStream_t st);
int rownorm_bwd_blocks(long long rows);
hipError_t launch_rownorm_act_bwd(const float* g, long long ldg, const int* gidx, const float* z, long long ldz, int C,
                                  const int* valid, const float* gamma, const float* beta, const float* stats, int act,
                                  float* dz, long long lddz, int Cpad, float* t_dy, float* t_dyx, long long rows,
                                  void* dz16, long long lddz16, const int* argrow, int z_lowp, hipStream_t st);
hipError_t launch_slot_reduce(const float* m, long long ldm, int C, const EdgeGraph& g, int S, const int* jc, int aggr,
                              float* out, long long ldo, int* ovf_row, int* deg, int* argrow, int post_act,
                              hipStream_t st);
hipError_t launch_slot_reduce_bwd(const float* gout, long long ldg, int C, const int* ic, const int* jc, long long rows,
                                  int aggr, const int* deg, const int* argrow, float* grows, long long ldr, int Cpad,
                                  hipStream_t st);
hipError_t launch_slot_sum(const float* m, long long ldm, int C, const EdgeGraph& g, int S, float* out, long long ldo,
                           hipStream_t st);
// pool.hip
hipError_t launch_pack_weights(const long long* desc, int ndesc, hipStream_t st);
// scratch (optional, pool_scratch_bytes(B, N, C)): a batch of a few huge events runs one workgroup per event SLICE (same result)
int event_slices_max(int B, int N);
long long pool_scratch_bytes(int B, int N, int C);
hipError_t launch_pool_fwd(const float* x, long long ldx, int C, const int* ptr, int B, int N, const int* codes, int ns,
                           float* out, int* argmin, int* argmax, hipStream_t st, void* scratch = nullptr);
hipError_t launch_pool_bwd(const float* gout, int C, const int* ptr, const int* batch, int N, const int* codes, int ns,
                           const int* argmin, const int* argmax, const float* gate, long long ldgate, void* dx,
                           long long lddx, int dx_lowp, hipStream_t st);
// generic.hip: BatchNorm1d over edge rows (masked by valid[r] >= 0)
int bn_blocks(long long rows);
hipError_t launch_bn_sums(int mode, int act, const float* z, long long ldz, long long rows, int C, const int* valid,
                          const float* g, long long ldg, const float* mean, const float* rstd, const float* gamma,
                          const float* beta, float* part, float* sums, hipStream_t st);
hipError_t launch_bn_finalize(const float* sums, const int* n_valid, int C, float eps, float* mean, float* rstd,
                              float* var_unbiased, hipStream_t st);
hipError_t launch_bn_act_fwd(const float* z, long long ldz, long long rows, int C, const int* valid, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, int act, void* a, long long lda,
                             int Cpad, int a_lowp, hipStream_t st);
hipError_t launch_bn_act_bwd(const float* g, long long ldg, const float* z, long long ldz, long long rows, int C,
                             const int* valid, const float* mean, const float* rstd, const float* gamma, const float* beta,
                             const float* sums, const int* n_valid, int act, void* dz, long long lddz, int Cpad, int dz_lowp,
                             hipStream_t st);
// attn.hip
hipError_t launch_attn_plan(const int* ptr, int B, int* plan, int sorted, hipStream_t st);
// (lowp: qkv / out / dout / dqkv are bf16 and the MFMA kernels run; else fp32 on the vector ALU)
hipError_t launch_attn_fwd(int lowp, const void* qkv, long long ld, int H, int DH, const int* ptr, const int* tile_ptr,
                           int B, int N, void* out, long long ldo, float* lse2, unsigned seed, unsigned thresh,
                           unsigned int* bits_r, unsigned int* bits_c, const long long* evoff, long long plane,
                           hipStream_t st);
hipError_t launch_attn_bwd(int lowp, const void* qkv, long long ld, int H, int DH, const int* ptr, const int* tile_ptr,
                           int B, int N, const void* out, long long ldo, const void* dout, long long lddo,
                           const float* lse2, float* delta, void* dqkv, long long lddq, unsigned seed, unsigned thresh,
                           const unsigned int* bits_r, const unsigned int* bits_c, const long long* evoff, long long plane,
                           hipStream_t st);
// attn_rel.hip: ragged attention with the spacetime bias of DeepIce recomputed per pair (fp32, head width 32)
bool rel_attn_supported(int DH);
hipError_t launch_rel_attn_fwd(const float* qkv, long long ld, const float* qp, long long ldqp, const float* xt, long long ldxt,
                               const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N,
                               float* out, long long ldo, float* u, long long ldu, float* lse2, hipStream_t st);
hipError_t launch_rel_attn_bwd(const float* qkv, long long ld, const float* qp, long long ldqp, const float* xt, long long ldxt,
                               const float* freq, int H, int DH, const int* ptr, const int* tile_ptr, int B, int N,
                               const float* out, long long ldo, const float* u, long long ldu, const float* dout,
                               long long lddo, const float* du, long long lddu, const float* lse2, float* delta,
                               float* dqkv, long long lddq, float* dqp, long long lddqp, hipStream_t st);
// generic.hip: dropout (+ residual add); thresh = round(p * 2^32)
hipError_t launch_dropout(const void* x, long long ldx, int x_lowp, const float* res, long long ldres, void* y, long long ldy,
                          int y_lowp, long long rows, int cols, unsigned seed, unsigned thresh, hipStream_t st);
}  // namespace gn
