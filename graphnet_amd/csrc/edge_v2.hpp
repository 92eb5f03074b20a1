// graphnet_amd/csrc/edge_v2.hpp — what edgeconv.hip (the dispatch) uses of edgeconv_v2.hip (persistent kernels) and
// dpre_compact.hip, and the switches both sides read.
#pragma once
#include "common.hpp"
#include "edge_plan.hpp"

namespace gn {
// edgeconv.hip
int edge_slots(int K);
EdgeSwitches edge_switches();
int device_cus();

// edgeconv_v2.hip: one launcher per pass.  variant = EdgePlan::variant (the kernels' template V); the caller has checked
// the envelope (EdgePlan::persistent) - outside it they return hipErrorNotSupported, as they do when an offset of the
// forward or dW2 kernel would not fit 32 bits.  tilevalid: variant 2 only (one 64-bit word per 64-row tile, bit = the row
// is an edge; written by the forward, read by dW2 and backward), else nullptr.
hipError_t launch_edge_fwd_v2(int variant, const EdgeGraph& g, const void* PQ, int H1p, int H1, const void* W2p, const float* b2,
                              int H2, void* out, long long ldo, float* coords, const CoordCols& cc, unsigned char* maskB,
                              unsigned long long* tilevalid, int num_cus, hipStream_t st);
// whether launch_edge_fwd_v2 takes the wave-specialised kernel for this layer (ldo: row pitch of `out` in elements)
bool edge_fwd_v2_ws(int variant, const EdgeGraph& g, int H1p, int H1, int H2, long long ldo, const EdgeSwitches& sw);
// slab: [parts][H2][H1], db2_part: [parts][H2] with parts = edge_dw2_v2_parts(); also writes hbits
int edge_dw2_v2_parts(int N, int K, int H1p, int num_cus);
hipError_t launch_edge_dw2_v2(int variant, const EdgeGraph& g, const void* PQ, int H1p, int H1, int H2, const void* gout,
                              long long ldg, const unsigned char* maskB, unsigned char* hbits,
                              const unsigned long long* tilevalid, float* slab, float* db2_part, int num_cus, hipStream_t st);
// needs hbits (the dW2 pass of the layer runs first).  cp != nullptr (variant 0 only): compact dpre, `dpre` is then unused
hipError_t launch_edge_bwd_v2(int variant, const EdgeGraph& g, int H1p, int H2, const void* gout, long long ldg,
                              const unsigned char* maskB, const unsigned char* hbits, const unsigned long long* tilevalid,
                              const void* W2Tp, int H2p, void* dpre, void* dP, long long ldp, int num_cus, hipStream_t st,
                              const BwdCompact* cp = nullptr);

// dpre_compact.hip
long long dpre_compact_tiles(int N, int K);
hipError_t launch_dpre_plan(int N, int K, int H1p, int H1, const unsigned char* hbits, unsigned short* rowoff, int* tilesize16,
                            int* tilebase, int* tmp, hipStream_t st);
hipError_t launch_dq_gather_cp(int N, int K, int H1p, int H1, const unsigned char* dpre_c, const int* tilebase,
                               const unsigned short* rowoff, const unsigned char* hbits, const void* dense_ovf_rows,
                               const int* rev_ptr, const int* rev_rows, const int* hubs, const int* nhubs, void* dQ, long long ldq,
                               hipStream_t st);
}  // namespace gn
