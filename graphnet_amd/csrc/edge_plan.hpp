// graphnet_amd/csrc/edge_plan.hpp — which kernels one fused EdgeConv layer runs.  Plain C++17 (no HIP include: a host
// compiler builds it alone, tests/test_edge_plan.py does).  Forward, dW2, dW2 reduction and backward of a layer read and
// write ONE `saved` buffer whose contents depend on the path, so all of them take their decisions from edge_plan() with
// the same arguments - nothing else under csrc/ decides.
#pragma once

namespace gn {

// Environment switches of the edge path; edge_switches() in edgeconv.hip is the only reader.
struct EdgeSwitches { bool disable_v2, ovf_gemm, dpre_compact; int edge_ws; int producers_first; };

struct EdgePlan {
    bool supported;      // act 1 (EdgeConvTito) has no tiled family: outside its envelope -> false
    bool persistent;     // table rows on edgeconv_v2.hip (else the tiled kernels of edgeconv.hip)
    int  variant;        // 0 relu, 1 leaky + max (Tito), 2 leaky + add (JINST) = the kernels' template V
    int  ovf;            // 0 no overflow list, 1 tiled overflow kernels, 2 GEMM path (launch_ovf_*)
    bool compact_shape;  // compact-dpre kernels can take this layer (the explicit entries)
    bool compact_model;  // ... and the model paths choose them (switch on)
    bool shape_persistent;  // the relu plan of this shape is persistent: the dW2 slabs are counted for the persistent
                            // kernels whatever the activation (act 2 outside its envelope spreads the tiled kernel over them)
};

// ---- shape envelopes of the persistent kernels (the only copy) -----------------------------------------------------
// relu (DynEdge): K <= 16 slots, the DynEdge layer widths
inline bool edge_v2_shape_ok(int K, int H1p, int H2) { return K <= 16 && H2 == 256 && (H1p == 128 || H1p == 352); }
// EdgeConvTito (leaky relu, max aggregation): the DynTrans layer sizes of the reference, (256, 256)
inline bool edge_v2_max_shape_ok(int K, int H1p, int H2) { return K <= 16 && H2 == 256 && H1p == 256; }
// DynEdgeJINST (leaky relu, add): hidden widths 337..352 have no wave-specialised forward (register budget)
inline bool edge_v2_leaky_shape_ok(int K, int H1p, int H1, int H2) {
    return edge_v2_shape_ok(K, H1p, H2) && (H1p == 128 || H1 <= 336);
}
// compact dpre: at most 43 real 8-column chunks of the 44, H1 <= 344 (the in-place compaction's LDS stage, edge_bwd_v2_kernel)
inline bool edge_bwd_v2_compact_ok(int K, int H1p, int H1) {
    return K <= 16 && (H1p == 128 || (H1p == 352 && (H1 + 7) / 8 <= 43));
}

// mode: 0 fp32 (tiled kernels only), 1 bf16.  act = variant.  H1 (real hidden width) decides for act 2 and for the
// compact_* fields only: the relu backward entry of the ABI does not carry it.  has_ovf: the graph has an overflow list.
inline EdgePlan edge_plan(int mode, int K, long long N, int H1p, int H1, int H2, int act, bool has_ovf, const EdgeSwitches& sw) {
    EdgePlan p = {};
    p.variant = act;
    if (act < 0 || act > 2) return p;
    const bool v2 = mode == 1 && !sw.disable_v2;
    p.shape_persistent = v2 && (act == 1 ? edge_v2_max_shape_ok(K, H1p, H2) : edge_v2_shape_ok(K, H1p, H2));
    if (act == 1) {                                        // table without overflow rows, or nothing
        p.supported = p.persistent = p.shape_persistent && !has_ovf;
        return p;
    }
    p.supported = true;
    p.persistent = p.shape_persistent && (act == 0 || edge_v2_leaky_shape_ok(K, H1p, H1, H2));
    // overflow rows on the GEMM kernels: they address the gathered [N][H1p] bf16 rows with 32-bit byte offsets.  Only next to
    // the persistent kernels (the tiled family takes table and overflow rows alike)
    if (has_ovf) p.ovf = p.persistent && sw.ovf_gemm && N * H1p * 2 < (1LL << 31) ? 2 : 1;
    p.compact_shape = p.persistent && act == 0 && edge_bwd_v2_compact_ok(K, H1p, H1);
    p.compact_model = p.compact_shape && sw.dpre_compact;
    return p;
}

}  // namespace gn
