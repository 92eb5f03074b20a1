"""ctypes binding of ``libgraphnet_amd.so`` (C ABI: ``include/graphnet_amd.h``).

The library is built in-tree by ``graphnet_amd/csrc/Makefile`` (``__graft_entry__.build()``).
There is no fallback: if the shared object is missing every device op raises.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from ctypes import c_char_p, c_float, c_int32, c_int64, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgraphnet_amd.so")
_lib = None
BUILT_IN_PROCESS = False      # True once build() has run make in this process (bench.py reports it)
ABI_VERSION = 7          # GN_ABI_VERSION of include/graphnet_amd.h these signatures mirror

P = c_void_p
I32 = c_int32
I64 = c_int64
U32 = c_uint32

# name -> (restype, argtypes); mirrors include/graphnet_amd.h one to one
SIGNATURES = {
    "gn_last_error": (c_char_p, []),
    "gn_abi_version": (I32, []),
    "gn_knn_graph": (I32, [P, I64, P, I32, P, P, I32, I32, I32, I32, P, P, P]),
    "gn_knn_ws_bytes": (I64, [I32, I32, I32]),
    "gn_knn_graph_ws": (I32, [P, I64, P, I32, P, P, I32, I32, I32, I32, P, P, P, P]),
    "gn_knn_plan": (I32, [P, I32, P, P]),
    "gn_minkowski_knn_graph": (I32, [P, I64, P, I32, I32, c_float, c_float, P, P, I32, I32, I32, P, P]),
    "gn_radius_work_ints": (I64, [I32, I32]),
    "gn_radius_graph": (I32, [P, I64, P, I32, c_float, P, P, I32, I32, I32, P, P, P, P]),
    "gn_percentile_work_ints": (I64, [I32, I32]),
    "gn_percentile_lds_max": (I32, []),
    "gn_percentile_clusters": (I32, [P, I64, I32, P, I32, P, I32, P, I32, P, I32, I32, P, I64, P, P, P]),
    "gn_dom_time_series_work_ints": (I64, [I32, I32]),
    "gn_dom_time_series": (I32, [P, I64, I32, I32, P, I32, P, I32, I32, I32, P, I64, P, P, P, P]),
    "gn_icemix_nodes": (I32, [P, I64, I32, I32, P, I32, I32, I32, I32, P, I32, U32, P, I32, P, I64, P, P, P]),
    "gn_gru_supported": (I32, [I32, I32]),
    "gn_gru_saved_floats": (I64, [I32, I32]),
    "gn_gru_bwd_work_floats": (I64, [I32, I32, I32]),
    "gn_gru_series_fwd": (I32, [P, I64, I32, I32, P, I32, I32, P, P, P, P, P, P, P]),
    "gn_gru_series_bwd": (I32, [P, P, P, I64, I32, I32, P, I32, I32, P, P, P, P, P, P, P]),
    "gn_dom_series_summary": (I32, [P, I64, I32, I32, P, I32, I32, P, I64, P]),
    "gn_scan_tmp_ints": (I64, [I64]),
    "gn_scan_i32": (I32, [P, P, I32, P, P, P]),
    "gn_ovf_compact": (I32, [P, I32, P, P, P, P, P, P]),
    "gn_edge_slots": (I32, [I32]),
    "gn_rev_build": (I32, [P, I32, I32, P, P, P, P, P, P, P]),
    "gn_rev_event_slices": (I32, [I32]),
    "gn_rev_build_events": (I32, [P, I32, I32, P, P, P, I32, P, P, P, P, P, P, P, P]),
    "gn_rev_pairs_ints": (I64, [I32, I32, I32]),
    "gn_rev_build_events_ws": (I32, [P, I32, I32, P, P, P, I32, P, P, P, P, P, P, P, P, P]),
    "gn_table_degree": (I32, [P, P, I32, I32, P, P]),
    "gn_table_to_edge_index": (I32, [P, P, I32, I32, P, I64, P, P]),
    "gn_edge_index_to_table": (I32, [P, I64, I32, I32, P, P, P, P, P]),
    "gn_ptr_to_batch": (I32, [P, I32, P, P]),
    "gn_standardize": (I32, [P, I64, I32, I32, P, P, P, P]),
    "gn_graph_globals": (I32, [P, I64, I32, P, I32, P, P, I32, P, P, P]),
    "gn_event_scratch_bytes": (I64, [I32, I32, I32]),
    "gn_graph_globals_ws": (I32, [P, I64, I32, P, I32, I32, P, P, I32, P, P, P, P]),
    "gn_segment_pool_fwd_ws": (I32, [P, I64, I32, P, I32, I32, P, I32, P, P, P, P, P]),
    "gn_concat_globals": (I32, [P, I64, I32, P, I32, P, I32, P, I32, I32, P]),
    "gn_linear_fwd": (I32, [I32, I32, P, I32, P, P, P, I32, P, I32, I32, I32, P, P, I32, I64, I32, I32, P, I64, I32, P]),
    "gn_linear_wgrad_parts": (I32, [I32, I32, I32, I32, P]),
    "gn_linear_wgrad": (I32, [I32, P, I32, I64, I32, I32, P, I32, P, P, I32, P, P, P, P, I32, P]),
    "gn_colsum_blocks": (I32, [I32]),
    "gn_colsum": (I32, [P, I64, I32, I32, P, P, I32, P]),
    "gn_reduce_slabs": (I32, [P, I32, I64, P, I32, P]),
    "gn_edgeconv_saved_bytes": (I64, [I32, I32, I32, I32]),
    "gn_edgeconv_fwd": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, P, P, I32, P, I64, P, P, I32, P, P]),
    "gn_edgeconv_bwd": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, P, I64, P, P, I32, P, P, I64, P]),
    "gn_edgeconv_dw2_slabs": (I32, [I32, I32, I32, I32, I32]),
    "gn_edgeconv_plan": (None, [I32, I32, I64, I32, I32, I32, I32, I32, P]),
    "gn_edgeconv_dw2": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, I32, P, I64, P, P, P, P]),
    "gn_edgeconv_dq_gather": (I32, [I32, P, I32, P, P, P, P, I32, P, I64, P]),
    "gn_edgeconv_max_supported": (I32, [I32, I32, I32, I32]),
    "gn_edgeconv_max_dw2_slabs": (I32, [I32, I32, I32]),
    "gn_edgeconv_max_fwd": (I32, [P, I32, I32, P, I32, P, P, I32, P, I64, P, P]),
    "gn_edgeconv_max_dw2": (I32, [P, I32, I32, P, I32, I32, I32, P, I64, P, P, P, P]),
    "gn_edgeconv_max_bwd": (I32, [P, I32, I32, I32, I32, P, I64, P, P, I32, P, P, I64, P]),
    "gn_edgeconv_dw2_reduce": (I32, [I32, P, I32, I32, I32, I32, I32, I32, P, P, P, P, P]),
    "gn_edgeconv_leaky_supported": (I32, [I32, I32, I32, I32, I32]),
    "gn_edgeconv_leaky_fwd": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, P, P, I32, P, I64, P, P, I32, P, P]),
    "gn_edgeconv_leaky_dw2": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, I32, P, I64, P, P, P, P]),
    "gn_edgeconv_leaky_bwd": (I32, [I32, P, P, P, P, I32, I32, P, I32, I32, I32, P, I64, P, P, I32, P, P, I64, P]),
    "gn_edge_rows": (I32, [P, P, P, P, I32, I32, P, P, P]),
    "gn_rows_compact": (I32, [P, P, I32, I32, P, P, P, P, P, P]),
    "gn_segment_rows_sum": (I32, [P, I64, I32, I32, P, P, I64, I32, P]),
    "gn_rev_rows_compact": (I32, [P, P, I32, I32, P, P, P, P, P]),
    "gn_edge_gather_pre": (I32, [P, I32, P, P, I64, I32, P, I32, P]),
    "gn_rownorm_act_fwd": (I32, [P, I64, I32, P, P, P, c_float, I32, P, I64, I32, P, I64, P, I64, I32, P]),
    "gn_rownorm_bwd_blocks": (I32, [I64]),
    "gn_rownorm_act_bwd": (I32, [P, I64, P, P, I64, I32, P, P, P, P, I32, P, I64, I32, P, P, I64, P, I64, P, I32, P]),
    "gn_slot_sum": (I32, [P, I64, I32, P, P, P, P, I32, I32, P, I64, P]),
    "gn_slot_reduce": (I32, [P, I64, I32, P, P, P, P, I32, I32, P, I32, P, I64, P, P, P, I32, P]),
    "gn_slot_reduce_bwd": (I32, [P, I64, I32, P, P, I64, I32, P, P, P, I64, I32, P]),
    "gn_pack_weights": (I32, [P, I32, P]),
    "gn_segment_pool_fwd": (I32, [P, I64, I32, P, I32, P, I32, P, P, P, P]),
    "gn_segment_pool_bwd": (I32, [P, I32, P, P, I32, P, I32, P, P, P, I64, P, I64, I32, P]),
    "gn_attention_plan": (I32, [P, I32, P, I32, P]),
    "gn_attention_fwd": (I32, [I32, P, I64, I32, I32, P, P, I32, I32, P, I64, P, U32, U32, P]),
    "gn_attention_bwd": (I32, [I32, P, I64, I32, I32, P, P, I32, I32, P, I64, P, I64, P, P, P, I64, U32, U32, P]),
    "gn_attention_fwd_bits": (I32, [P, I64, I32, I32, P, P, I32, I32, P, I64, P, U32, U32, P, P, P, I64, P]),
    "gn_attention_bwd_bits": (I32, [P, I64, I32, I32, P, P, I32, I32, P, I64, P, I64, P, P, P, I64, U32, P, P, P, I64, P]),
    "gn_rel_attention_supported": (I32, [I32]),
    "gn_rel_attention_fwd": (I32, [P, I64, P, I64, P, I64, P, I32, I32, P, P, I32, I32, P, I64, P, I64, P, P]),
    "gn_rel_attention_bwd": (I32, [P, I64, P, I64, P, I64, P, I32, I32, P, P, I32, I32, P, I64, P, I64, P, I64, P, I64, P, P,
                                   P, I64, P, I64, P]),
    "gn_bn_blocks": (I64, [I64]),
    "gn_bn_sums": (I32, [I32, I32, P, I64, I64, I32, P, P, I64, P, P, P, P, P, P, P]),
    "gn_bn_finalize": (I32, [P, P, I32, c_float, P, P, P, P]),
    "gn_bn_act_fwd": (I32, [P, I64, I64, I32, P, P, P, P, P, I32, P, I64, I32, I32, P]),
    "gn_bn_act_bwd": (I32, [P, I64, P, I64, I64, I32, P, P, P, P, P, P, P, I32, P, I64, I32, I32, P]),
    "gn_dropout": (I32, [P, I64, I32, P, I64, P, I64, I32, I64, I32, U32, U32, P]),
    "gn_edgeconv_saved_offsets": (None, [I32, I32, I32, I32, P]),
    "gn_edgeconv_dpre_compact_supported": (I32, [I32, I32, I32, I32, I32]),
    "gn_edgeconv_dpre_plan_bytes": (I64, [I32, I32]),
    "gn_edgeconv_dpre_compact_bytes": (I64, [I32, I32, I32]),
    "gn_edgeconv_dpre_plan": (I32, [I32, I32, I32, I32, I32, P, P, P]),
    "gn_edgeconv_bwd_compact": (I32, [P, P, P, P, I32, I32, P, I32, I32, I32, P, I64, P, P, I32, P, P, P, P, I64, P]),
    "gn_edgeconv_dq_gather_compact": (I32, [I32, I32, I32, I32, I32, P, P, P, P, P, P, P, P, P, I64, P]),
    # one entry per backbone pass (descriptor structs: graphnet_amd/step.py)
    "gn_dynedge_wws_bytes": (I64, [P]),
    "gn_dynedge_ws_bytes": (I64, [P]),
    "gn_dynedge_bwd_ws_bytes": (I64, [P]),
    "gn_dynedge_fwd": (I32, [P, P, P]),
    "gn_dynedge_bwd": (I32, [P, P, P, I64, P]),
    "gn_step_last_error": (c_char_p, []),
    "gn_step_timers_enable": (None, [I32]),
    "gn_step_timers_read": (I64, [P, I64]),
}


def build(verbose: bool = False) -> str:
    """Compile every HIP source for gfx950 into ``libgraphnet_amd.so`` (in-tree).  Serialised by a file lock: N
    ranks starting on a fresh checkout must not run ``make`` on the same ``build/*.o`` at once - the first one builds,
    the others wait and find everything up to date."""
    import fcntl
    global BUILT_IN_PROCESS
    BUILT_IN_PROCESS = True
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j", "6"]
    with open(os.path.join(_HERE, "csrc", ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError("building libgraphnet_amd.so failed:\n" + res.stdout[-4000:])
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load the C-ABI library (never falls back to anything else)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and os.environ.get("GN_NO_AUTOBUILD") != "1" and \
                os.path.exists(os.path.join(_HERE, "csrc", "Makefile")):
            build_error = None
            try:                                    # a checkout without build artefacts: compile once (hipcc, ~1 min)
                build()
            except Exception as exc:                # no hipcc / compile error: chained into the error below
                build_error = exc
        else:
            build_error = None
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
                "graphnet_amd has no CPU fallback for device ops."
            ) from build_error
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        if handle.gn_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} has ABI version {handle.gn_abi_version()}, this package binds version "
                               f"{ABI_VERSION}: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(lib().gn_last_error().decode())
