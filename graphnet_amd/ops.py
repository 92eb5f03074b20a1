"""Tensor-level wrappers over the C ABI (``include/graphnet_amd.h``).

PyTorch supplies device memory and the HIP stream; every computation on the DynEdge path is a
kernel of ``libgraphnet_amd.so``.  All functions require CUDA(HIP) tensors and raise
``RuntimeError`` if the library is missing — there is no CPU path here by design.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

MODE_F32 = 0
MODE_BF16 = 1
POOL_CODES = {"min": 0, "max": 1, "sum": 2, "mean": 3}


# ---- optional per-op HIP-event timers (bench.py's live roofline measurement) --------------
_TIMERS = None


def enable_timers(on: bool = True) -> None:
    """Record a HIP event pair on the launch stream around every C-ABI op."""
    global _TIMERS
    _TIMERS = {} if on else None
    _lib.lib().gn_step_timers_enable(1 if on else 0)        # ... and inside the one-call entries (csrc/step.hip)


class _timed:
    """``detail``: a second key (op + shape) under which the same event pair is also listed, so that a caller can
    price ONE kernel shape (bench.py's roofline) instead of the whole op group."""

    def __init__(self, name: str, detail: Optional[str] = None):
        self.name, self.detail = name, detail

    def __enter__(self):
        if _TIMERS is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if _TIMERS is not None:
            self.ev[1].record()
            _TIMERS.setdefault(self.name, []).append(self.ev)
            if self.detail is not None:
                _TIMERS.setdefault("@" + self.detail, []).append(self.ev)
        return False


def timer_summary(detail: bool = False) -> dict:
    """name -> (launches, total milliseconds); synchronises.  ``detail=True``: the per-shape entries instead
    (``"edgeconv_dw2[352x256]"`` = H1p x H2)."""
    torch.cuda.synchronize()
    out = {(k[1:] if detail else k): (len(v), sum(a.elapsed_time(b) for a, b in v))
           for k, v in (_TIMERS or {}).items() if k.startswith("@") == detail}
    if _TIMERS is not None:                # events recorded inside gn_dynedge_fwd / gn_dynedge_bwd: "name[AxB]" or "name"
        from .step import timers_read
        for name, (n, ms) in timers_read().items():
            key = name if detail else name.split("[", 1)[0]
            if detail and "[" not in name:
                continue
            n0, ms0 = out.get(key, (0, 0.0))
            out[key] = (n0 + n, ms0 + ms)
    return out


def mode_dtype(mode: int) -> torch.dtype:
    return torch.float32 if mode == MODE_F32 else torch.bfloat16


def _st() -> int:
    """Raw handle of torch's current HIP stream (called once per kernel launch: the private fast getter
    costs ~0.3 us, ``torch.cuda.current_stream().cuda_stream`` ~10 us)."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())
    except AttributeError:                                   # pragma: no cover - other torch builds
        return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(t: Tensor, dtype: torch.dtype, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: graphnet_amd device ops need a HIP tensor (got {t.device}); no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")


def _rows(t: Tensor, name: str) -> int:
    """Row pitch (elements) of a 2-D tensor whose rows are contiguous."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: need a 2-D tensor with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------ graph
@dataclass
class NeighbourTable:
    """One layer's graph: fixed-stride table + overflow list (+ lazily built reverse lists)."""

    nbr: Tensor                 # [N, K] int32, -1 padded
    ovf: Optional[Tensor]       # [N] int32 (-1 = none) or None in strict mode
    ovf_centre: Optional[Tensor]
    ovf_src: Optional[Tensor]
    ovf_cnt: Optional[Tensor]   # [1] int32 on device
    K: int
    rev_ptr: Optional[Tensor] = None
    rev_rows: Optional[Tensor] = None
    rev_hubs: Optional[Tensor] = None      # nodes with 65..16384 in-edges (sorted lists) ...
    rev_nhubs: Optional[Tensor] = None     # ... and their number (int32[>=1], element 0)

    @property
    def N(self) -> int:
        return int(self.nbr.shape[0])

    @property
    def S(self) -> int:
        return int(_lib.lib().gn_edge_slots(self.K))

    @property
    def rows(self) -> int:
        """Upper bound of edge rows (table rows + one overflow row per node)."""
        return self.N * self.S + self.N

    def c_args(self):
        return (_p(self.nbr), _p(self.ovf_centre), _p(self.ovf_src), _p(self.ovf_cnt), self.N, self.K)

    def build_reverse(self) -> None:
        if self.rev_ptr is not None:
            return
        L = _lib.lib()
        N, dev = self.N, self.nbr.device
        ev_ptr = getattr(self, "event_ptr", None)
        B = int(ev_ptr.shape[0]) - 1 if ev_ptr is not None else 0
        # edges never leave an event (built by knn_graph): per-event build with LDS counters, one workgroup per
        # (event, slice of its sources) - a handful of 10^4-pulse events (BASELINE configs[4]) is cut into enough
        # slices to fill the chip
        if ev_ptr is not None and (self.ovf is None or getattr(self, "ovf_pos", None) is not None) and B >= 1:
            G = B * int(L.gn_rev_event_slices(B))
            rev_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
            rev_rows = torch.empty(max(N * self.K + N, 1), dtype=torch.int32, device=dev)
            ev = torch.empty(2 * (G + 1), dtype=torch.int32, device=dev)
            scratch = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
            hubs = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
            tmp = torch.empty(int(L.gn_scan_tmp_ints(max(G, 1))) + 1, dtype=torch.int32, device=dev)
            nhubs = tmp[-1:]
            npairs = int(L.gn_rev_pairs_ints(B, N, self.K))      # > 0: few, huge events - bucketed build
            pairs = torch.empty(npairs, dtype=torch.int32, device=dev) if npairs > 0 else None
            with _timed("rev_build"):
                _lib.check(L.gn_rev_build_events_ws(_p(self.nbr), N, self.K, _p(self.ovf), _p(getattr(self, "ovf_pos", None)),
                                                    _p(ev_ptr), B, _p(rev_ptr), _p(rev_rows), _p(ev), _p(scratch), _p(hubs),
                                                    _p(nhubs), _p(tmp), _p(pairs), _st()))
            self.rev_ptr, self.rev_rows = rev_ptr, rev_rows
            self.rev_hubs, self.rev_nhubs = hubs, nhubs
            return
        rev_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        cursor = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        tmp = torch.empty(int(L.gn_scan_tmp_ints(N)), dtype=torch.int32, device=dev)
        rev_rows = torch.empty(max(N * self.K + N, 1), dtype=torch.int32, device=dev)
        with _timed("rev_build"):
            _lib.check(L.gn_rev_build(_p(self.nbr), N, self.K, _p(self.ovf_src), _p(self.ovf_cnt), _p(rev_ptr),
                                      _p(cursor), _p(tmp), _p(rev_rows), _st()))
        self.rev_ptr, self.rev_rows = rev_ptr, rev_rows
        self.rev_hubs, self.rev_nhubs = cursor, tmp        # hub list / its length, left there by gn_rev_build

    def edge_index(self) -> Tensor:
        """Materialise PyG-style ``edge_index[2,E]`` int64 (API boundary only; syncs)."""
        L = _lib.lib()
        N, dev = self.N, self.nbr.device
        deg = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(L.gn_table_degree(_p(self.nbr), _p(self.ovf), N, self.K, _p(deg), _st()))
        off = torch.empty(N, dtype=torch.int32, device=dev)
        tot = torch.zeros(1, dtype=torch.int32, device=dev)
        tmp = torch.empty(int(L.gn_scan_tmp_ints(N)), dtype=torch.int32, device=dev)
        _lib.check(L.gn_scan_i32(_p(deg), _p(off), N, _p(tmp), _p(tot), _st()))
        E = int(tot.item())
        ei = torch.empty((2, E), dtype=torch.int64, device=dev)
        _lib.check(L.gn_table_to_edge_index(_p(self.nbr), _p(self.ovf), N, self.K, _p(off), E, _p(ei), _st()))
        return ei


def _finish_table(nbr: Tensor, ovf: Optional[Tensor], K: int) -> NeighbourTable:
    if ovf is None:
        return NeighbourTable(nbr, None, None, None, None, K)
    L = _lib.lib()
    N, dev = int(nbr.shape[0]), nbr.device
    work = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    tmp = torch.empty(int(L.gn_scan_tmp_ints(N)), dtype=torch.int32, device=dev)
    oc = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    os_ = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.gn_ovf_compact(_p(ovf), N, _p(work), _p(tmp), _p(oc), _p(os_), _p(cnt), _st()))
    t = NeighbourTable(nbr, ovf, oc, os_, cnt, K)
    t.ovf_pos = work            # exclusive scan of the overflow flags: index of every centre's overflow row
    return t


def knn_plan(ptr: Tensor, n_nodes: int) -> Tensor:
    """Query-tile plan of a batch (``gn_knn_plan``): build once, pass to every ``knn_graph`` of the batch.
    int32 ``[B+1]`` tile offsets, then the count and ids of the tiles of events above 1024 pulses."""
    _need(ptr, torch.int32, "ptr")
    B = int(ptr.shape[0]) - 1
    plan = torch.empty(B + 2 + int(n_nodes) // 64 + B, dtype=torch.int32, device=ptr.device)
    _lib.check(_lib.lib().gn_knn_plan(_p(ptr), B, _p(plan), _st()))
    return plan


def knn_graph(x: Tensor, cols: Sequence[int], batch: Tensor, ptr: Tensor, k: int,
              strict: bool = False, plan: Optional[Tensor] = None, sweep: bool = False) -> NeighbourTable:
    """Batched exact k-NN on ``x[:, cols]`` (fp32) inside each event.  ``sweep=True`` hands ``gn_knn_graph_ws`` the scratch
    of the large-event path (sort along a space-filling curve + bounding-box pruning, events of 1025..16384 pulses in
    batches that average >= 512 per event): the same table, faster where pulses coincide or cluster - the graph on the
    DETECTOR coordinates (a DOM's pulses share a position: 2.5x at 10^4 pulses per event); on the learned coordinates of
    the later layers it measured slower than the exhaustive scan, so those callers leave it off."""
    if plan is None:
        plan = knn_plan(ptr, int(x.shape[0]))
    _need(x, torch.float32, "x"); _need(batch, torch.int32, "batch"); _need(ptr, torch.int32, "ptr")
    N = int(x.shape[0])
    ld = _rows(x, "x")
    nbr = torch.empty((N, k), dtype=torch.int32, device=x.device)
    ovf = None if strict else torch.empty(max(N, 1), dtype=torch.int32, device=x.device)
    c = (ctypes.c_int32 * len(cols))(*[int(v) for v in cols])
    B = int(ptr.shape[0]) - 1
    # scratch of the large-event path (sorted sweep): only batches that average >= 512 pulses per event use it
    ws = None
    if sweep and B > 0 and N >= 512 * B:
        ws = torch.empty(int(_lib.lib().gn_knn_ws_bytes(B, N, len(cols))), dtype=torch.uint8, device=x.device)
    with _timed("knn_graph"):
        _lib.check(_lib.lib().gn_knn_graph_ws(_p(x), ld, ctypes.cast(c, ctypes.c_void_p), len(cols), _p(ptr),
                                              _p(plan), B, N, k, 1 if strict else 0, _p(nbr), _p(ovf), _p(ws), _st()))
    table = _finish_table(nbr, None if strict else ovf[:N] if N else ovf, k)
    table.event_ptr = ptr       # every edge stays inside its event: the reverse lists can be built event by event
    return table


def minkowski_knn_graph(x: Tensor, space_cols: Sequence[int], time_col: int, c: float, time_like_weight: float,
                        batch: Tensor, ptr: Tensor, k: int, plan: Optional[Tensor] = None) -> NeighbourTable:
    """Batched k-NN under the Minkowski metric inside each event (``gn_minkowski_knn_graph``; the reference's
    ``MinkowskiKNNEdges``, ``graphs/edges/minkowski.py:66-99``): ``m = |dx|^2 - (c dt)^2`` on ``x[:, space_cols]`` and
    ``x[:, time_col]``, negative (time-like) ``m`` scaled by ``-time_like_weight``, per centre the ``k`` smallest
    ``(m, j)`` with the centre excluded by index.  Returns the strict table (degree ``min(k, n - 1)``, no overflow
    column).  Events of any size are scanned exhaustively: the sorted sweep's pruning bound is Euclidean."""
    if plan is None:
        plan = knn_plan(ptr, int(x.shape[0]))
    _need(x, torch.float32, "x"); _need(batch, torch.int32, "batch"); _need(ptr, torch.int32, "ptr")
    N = int(x.shape[0])
    ld = _rows(x, "x")
    if any(not 0 <= int(v) < int(x.shape[1]) for v in list(space_cols) + [time_col]):
        raise ValueError(f"minkowski_knn_graph: columns {list(space_cols)} / {time_col} outside x[:, :{int(x.shape[1])}]")
    nbr = torch.empty((N, k), dtype=torch.int32, device=x.device)
    sc = (ctypes.c_int32 * len(space_cols))(*[int(v) for v in space_cols])
    B = int(ptr.shape[0]) - 1
    with _timed("minkowski_knn_graph"):
        _lib.check(_lib.lib().gn_minkowski_knn_graph(_p(x), ld, ctypes.cast(sc, ctypes.c_void_p), len(space_cols),
                                                     int(time_col), float(c), float(time_like_weight), _p(ptr), _p(plan),
                                                     B, N, k, _p(nbr), _st()))
    table = _finish_table(nbr, None, k)
    table.event_ptr = ptr       # every edge stays inside its event: the reverse lists can be built event by event
    return table


def radius_graph(x: Tensor, cols: Sequence[int], r: float, batch: Tensor, ptr: Tensor, max_num_neighbours: int = 32,
                 plan: Optional[Tensor] = None) -> NeighbourTable:
    """Batched radius graph on ``x[:, cols]`` (fp32) inside each event (``gn_radius_graph``; the reference's
    ``RadialEdges``, ``graphs/edges/edges.py:83-117``): edge ``j -> i`` iff ``j != i`` and ``d2 < r*r`` (strict), every
    centre's sources ascending by index; a centre with more than ``max_num_neighbours`` in-radius pulses keeps the
    nearest ones in the total order ``(d2, j)``.  Returns the strict table (no overflow column), as wide as the graph
    needs - ``K = max(1, min(max_num_neighbours, deg.max()))``, one read-back - with the uncapped in-radius counts as
    the attribute ``deg`` (int32 ``[N]``): ``(table.deg > max_num_neighbours).sum()`` centres hit the cap."""
    if plan is None:
        plan = knn_plan(ptr, int(x.shape[0]))
    _need(x, torch.float32, "x"); _need(batch, torch.int32, "batch"); _need(ptr, torch.int32, "ptr")
    N = int(x.shape[0])
    ld = _rows(x, "x")
    cap = int(max_num_neighbours)
    if any(not 0 <= int(v) < int(x.shape[1]) for v in cols):
        raise ValueError(f"radius_graph: columns {list(cols)} outside x[:, :{int(x.shape[1])}]")
    nbr = torch.empty((N, max(cap, 0)), dtype=torch.int32, device=x.device)
    deg = torch.empty(N, dtype=torch.int32, device=x.device)
    c = (ctypes.c_int32 * len(cols))(*[int(v) for v in cols])
    B = int(ptr.shape[0]) - 1
    L = _lib.lib()
    work = torch.empty(max(int(L.gn_radius_work_ints(B, N)), 1), dtype=torch.int32, device=x.device)
    with _timed("radius_graph"):
        _lib.check(L.gn_radius_graph(_p(x), ld, ctypes.cast(c, ctypes.c_void_p), len(cols), float(r), _p(ptr), _p(plan),
                                     B, N, cap, _p(nbr), _p(deg), _p(work), _st()))
    K = max(1, min(cap, int(deg.max().item()) if N and B > 0 else 0))
    if N == 0 or B <= 0:
        nbr = torch.full((N, K), -1, dtype=torch.int32, device=x.device)
    table = _finish_table(nbr[:, :K].contiguous(), None, K)
    table.event_ptr = ptr       # every edge stays inside its event: the reverse lists can be built event by event
    table.deg = deg
    return table


def percentile_clusters(x: Tensor, ptr: Tensor, cluster_cols: Sequence[int], summ_cols: Sequence[int],
                        percentiles: Sequence[float], add_counts: bool = True,
                        out_pitch: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Batched DOM clustering with percentile features (``gn_percentile_clusters``; the reference's
    ``PercentileClusters``, ``graphs/nodes/nodes.py:135-217``): inside each event of ``ptr`` (int32 ``[B + 1]``) the rows
    of ``x`` (fp32) with equal ``cluster_cols`` become one node ``[cluster columns | percentiles of every column of
    summ_cols | log10(count)]``, nodes ascending in the reference's lexsort order.  Returns ``(nodes[M, W], node_ptr int32
    [B + 1])``: one call, one read-back (``M``); ``nodes`` is a view of the first ``M`` rows of the ``N``-row buffer the
    kernel wrote (``out_pitch``: its row pitch, ``W`` by default).  The contract is spelled out in
    ``include/graphnet_amd.h``."""
    _need(x, torch.float32, "x"); _need(ptr, torch.int32, "ptr")
    N, B = int(x.shape[0]), int(ptr.shape[0]) - 1
    C, S, P = len(cluster_cols), len(summ_cols), len(percentiles)
    W = C + S * P + (1 if add_counts else 0)
    ldo = W if out_pitch is None else int(out_pitch)
    if ldo < W:
        raise ValueError(f"percentile_clusters: out_pitch {ldo} < {W} columns")
    if any(not 0 <= int(v) < int(x.shape[1]) for v in list(cluster_cols) + list(summ_cols)):
        raise ValueError(f"percentile_clusters: columns {list(cluster_cols)} / {list(summ_cols)} outside x[:, :{int(x.shape[1])}]")
    if N == 0 or B <= 0:
        return (torch.empty((0, ldo), dtype=torch.float32, device=x.device)[:, :W],
                torch.zeros(max(B, 0) + 1, dtype=torch.int32, device=x.device))
    ld = _rows(x, "x")
    cl = (ctypes.c_int32 * C)(*[int(v) for v in cluster_cols])
    sm = (ctypes.c_int32 * S)(*[int(v) for v in summ_cols])
    q = (ctypes.c_double * P)(*[float(v) / 100.0 for v in percentiles])      # numpy's true_divide(q, 100), fp64
    L = _lib.lib()
    out = torch.empty((N, ldo), dtype=torch.float32, device=x.device)
    node_ptr = torch.empty(B + 1, dtype=torch.int32, device=x.device)
    # int64 elements: the sort keys at the front of `work` are 8 bytes wide
    work = torch.empty((int(L.gn_percentile_work_ints(B, N)) + 1) // 2, dtype=torch.int64, device=x.device)
    with _timed("percentile_clusters"):
        _lib.check(L.gn_percentile_clusters(_p(x), ld, N, _p(ptr), B, ctypes.cast(cl, ctypes.c_void_p), C,
                                            ctypes.cast(sm, ctypes.c_void_p), S, ctypes.cast(q, ctypes.c_void_p), P,
                                            1 if add_counts else 0, _p(out), ldo, _p(node_ptr), _p(work), _st()))
    M = int(node_ptr[B].item())
    return out[:M, :W], node_ptr


def dom_time_series(x: Tensor, ptr: Tensor, id_cols: Sequence[int], time_col: int, charge_col: int = -1,
                    out_pitch: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Batched DOM time series (``gn_dom_time_series``; the reference's ``NodeAsDOMTimeSeries``,
    ``graphs/nodes/nodes.py:220-306``): inside each event of ``ptr`` (int32 ``[B + 1]``) the rows of ``x`` (fp32) are
    grouped by ``id_cols`` and ordered by time inside a group, the time column is shifted to start at 0, the charge column
    is raised to ``10^x`` (``charge_col = -1``: a column of ones is appended) and ``new_node_col`` marks every group's first
    row.  Returns ``(rows[N, W], series_ptr int32 [M + 1], dom_ptr int32 [B + 1])``: one call, one read-back (``M``).  The
    contract is spelled out in ``include/graphnet_amd.h``."""
    _need(x, torch.float32, "x"); _need(ptr, torch.int32, "ptr")
    N, F, B = int(x.shape[0]), int(x.shape[1]), int(ptr.shape[0]) - 1
    C = len(id_cols)
    W = F + (1 if charge_col < 0 else 0) + 1
    ldo = W if out_pitch is None else int(out_pitch)
    if ldo < W:
        raise ValueError(f"dom_time_series: out_pitch {ldo} < {W} columns")
    ld = _rows(x, "x") if N > 0 else max(F, 1)
    idc = (ctypes.c_int32 * max(C, 1))(*[int(v) for v in id_cols])
    L = _lib.lib()
    out = torch.empty((N, ldo), dtype=torch.float32, device=x.device)
    series_ptr = torch.empty(N + 1, dtype=torch.int32, device=x.device)
    dom_ptr = torch.empty(max(B, 0) + 1, dtype=torch.int32, device=x.device)
    # int64 elements: the sort keys at the front of `work` are 8 bytes wide
    work = torch.empty((max(int(L.gn_dom_time_series_work_ints(max(B, 0), N)), 0) + 1) // 2 + 1, dtype=torch.int64, device=x.device)
    with _timed("dom_time_series"):
        _lib.check(L.gn_dom_time_series(_p(x), ld, F, N, _p(ptr), B, ctypes.cast(idc, ctypes.c_void_p), C, int(time_col),
                                        int(charge_col), _p(out), ldo, _p(series_ptr), _p(dom_ptr), _p(work), _st()))
    if N == 0 or B <= 0:
        dom_ptr.zero_()
        return out[:, :W], series_ptr[:1], dom_ptr
    M = int(dom_ptr[B].item())
    return out[:, :W], series_ptr[:M + 1], dom_ptr


def icemix_nodes(x: Tensor, ptr: Tensor, max_pulses: int, hlc_col: int = -1, z_col: int = -1,
                 table: Optional[Tensor] = None, seed: int = 0, event_ids: Optional[Tensor] = None, key_bits: int = 32,
                 out_pitch: Optional[int] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Batched pulse sampling with ice properties (``gn_icemix_nodes``; the reference's ``IceMixNodes``,
    ``graphs/nodes/nodes.py:309-453``): every event of ``ptr`` (int32 ``[B + 1]``) keeps a uniformly random ``max_pulses``
    of its rows of ``x`` (fp32) in their order, column ``hlc_col`` becomes its logical not and, with ``z_col >= 0``, two
    columns interpolated from ``table`` (fp64 ``[3, T]`` on the device: knots, scattering, absorption) are appended.
    Returns ``(nodes[M, W], node_ptr int32 [B + 1], ids int32 [M])``, ``ids`` the row of ``x`` behind every node: one call,
    one read-back (``M``).  ``event_ids`` (``[B]`` integers, by default the event ordinals) name the random stream of each
    event; ``key_bits`` below 32 only serves tests.  The contract is spelled out in ``include/graphnet_amd.h``."""
    _need(x, torch.float32, "x"); _need(ptr, torch.int32, "ptr")
    N, F, B = int(x.shape[0]), int(x.shape[1]), int(ptr.shape[0]) - 1
    W = F + (2 if z_col >= 0 else 0)
    ldo = W if out_pitch is None else int(out_pitch)
    if ldo < W:
        raise ValueError(f"icemix_nodes: out_pitch {ldo} < {W} columns")
    T = 0
    if z_col >= 0:
        if table is None:
            raise ValueError("icemix_nodes: the ice columns need table[3, T]")
        _need(table, torch.float64, "table")
        T = int(table.shape[1]) if table.dim() == 2 and table.shape[0] == 3 and table.is_contiguous() else -1
        if not 2 <= T <= 1024:
            raise ValueError(f"icemix_nodes: table must be a contiguous fp64 [3, T] with 2 <= T <= 1024, got {tuple(table.shape)}")
    if event_ids is not None:
        if int(event_ids.numel()) != max(B, 0):
            raise ValueError(f"icemix_nodes: event_ids has {int(event_ids.numel())} entries for {B} events")
        # uint32 values in an int32 tensor (two's complement): torch has no arithmetic on uint32
        event_ids = (event_ids.to(device=x.device, dtype=torch.int64) & 0xFFFFFFFF).to(torch.int32).contiguous()
    if N == 0 or B <= 0:
        return (torch.empty((0, ldo), dtype=torch.float32, device=x.device)[:, :W],
                torch.zeros(max(B, 0) + 1, dtype=torch.int32, device=x.device),
                torch.empty(0, dtype=torch.int32, device=x.device))
    ld = _rows(x, "x")
    out = torch.empty((N, ldo), dtype=torch.float32, device=x.device)
    node_ptr = torch.empty(B + 1, dtype=torch.int32, device=x.device)
    ids = torch.empty(N, dtype=torch.int32, device=x.device)
    with _timed("icemix_nodes"):
        _lib.check(_lib.lib().gn_icemix_nodes(_p(x), ld, F, N, _p(ptr), B, int(max_pulses), int(hlc_col), int(z_col),
                                              _p(table) if z_col >= 0 else None, T, int(seed) & 0xFFFFFFFF, _p(event_ids),
                                              int(key_bits), _p(out), ldo, _p(node_ptr), _p(ids), _st()))
    M = int(node_ptr[B].item())
    return out[:M, :W], node_ptr, ids[:M]


def gru_supported(input_size: int, hidden_size: int) -> bool:
    return bool(_lib.lib().gn_gru_supported(int(input_size), int(hidden_size)))


def gru_series_fwd(xs: Tensor, series_ptr: Tensor, w_ih: Tensor, w_hh: Tensor, b_ih: Tensor, b_hh: Tensor,
                   save: bool = True) -> Tuple[Tensor, Optional[Tensor]]:
    """Final hidden state of a GRU over every series of ``xs[T, I]`` (``gn_gru_series_fwd``; series ``s`` = rows
    ``series_ptr[s] .. series_ptr[s + 1]``): ``(out[M, H], saved)``; fp32 whatever the compute mode.  Raises outside the
    envelope of ``gn_gru_supported`` - there is no other implementation."""
    for t, name in ((xs, "xs"), (w_ih, "weight_ih"), (w_hh, "weight_hh"), (b_ih, "bias_ih"), (b_hh, "bias_hh")):
        _need(t, torch.float32, name)
    _need(series_ptr, torch.int32, "series_ptr")
    T, I, M, H = int(xs.shape[0]), int(xs.shape[1]), int(series_ptr.shape[0]) - 1, int(w_hh.shape[1])
    if tuple(w_ih.shape) != (3 * H, I) or tuple(w_hh.shape) != (3 * H, H):
        raise ValueError(f"gru_series_fwd: weights {tuple(w_ih.shape)} / {tuple(w_hh.shape)} do not fit xs[:, {I}]")
    L = _lib.lib()
    out = torch.empty((M, H), dtype=torch.float32, device=xs.device)
    saved = torch.empty(max(int(L.gn_gru_saved_floats(T, H)), 4), dtype=torch.float32, device=xs.device) if save else None
    with _timed("gru_series_fwd"):
        _lib.check(L.gn_gru_series_fwd(_p(xs), _rows(xs, "xs") if T > 0 else I, T, I, _p(series_ptr), M, H,
                                       _p(w_ih.contiguous()), _p(w_hh.contiguous()), _p(b_ih.contiguous()),
                                       _p(b_hh.contiguous()), _p(out), _p(saved), _st()))
    return out, saved


def gru_series_bwd(dout: Tensor, saved: Tensor, xs: Tensor, series_ptr: Tensor, w_hh: Tensor):
    """``(dW_ih[3H, I], db_ih, dW_hh[3H, H], db_hh)`` of :func:`gru_series_fwd` (``gn_gru_series_bwd``)."""
    _need(dout, torch.float32, "dout"); _need(saved, torch.float32, "saved"); _need(xs, torch.float32, "xs")
    T, I, M, H = int(xs.shape[0]), int(xs.shape[1]), int(series_ptr.shape[0]) - 1, int(w_hh.shape[1])
    L = _lib.lib()
    dev = xs.device
    Ip = round_up(I, 4)
    dw_ih = torch.empty((3 * H, Ip), dtype=torch.float32, device=dev)
    dw_hh = torch.empty((3 * H, H), dtype=torch.float32, device=dev)
    db_ih = torch.empty(3 * H, dtype=torch.float32, device=dev)
    db_hh = torch.empty(3 * H, dtype=torch.float32, device=dev)
    nwork = int(L.gn_gru_bwd_work_floats(T, I, H))
    if nwork < 0:
        raise RuntimeError(f"gru_series_bwd: input size {I} / hidden size {H} outside the envelope of gn_gru_supported")
    work = torch.empty(max(nwork, 4), dtype=torch.float32, device=dev)
    with _timed("gru_series_bwd"):
        _lib.check(L.gn_gru_series_bwd(_p(dout.contiguous()), _p(saved), _p(xs), _rows(xs, "xs") if T > 0 else I, T, I,
                                       _p(series_ptr), M, H, _p(w_hh.contiguous()), _p(dw_ih), _p(db_ih), _p(dw_hh),
                                       _p(db_hh), _p(work), _st()))
    return dw_ih[:, :I], db_ih, dw_hh, db_hh


def dom_series_summary(x: Tensor, series_ptr: Tensor, n_cols: int, charge_col: int) -> Tensor:
    """One row per series (``gn_dom_series_summary``): the series' first row, columns ``[0, n_cols)``, with ``charge_col``
    replaced by ``asinh`` of the series' summed charge."""
    _need(x, torch.float32, "x"); _need(series_ptr, torch.int32, "series_ptr")
    N, M = int(x.shape[0]), int(series_ptr.shape[0]) - 1
    out = torch.empty((M, n_cols), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().gn_dom_series_summary(_p(x), _rows(x, "x") if N > 0 else int(x.shape[1]), int(n_cols), N,
                                                _p(series_ptr), M, int(charge_col), _p(out), max(n_cols, 1), _st()))
    return out


def table_from_edge_index(edge_index: Tensor, N: int, K: int) -> NeighbourTable:
    """Loader-supplied ``edge_index`` -> neighbour table.  PyG's ``EdgeConv`` takes edges in any order and of any
    in-degree, so this does too: edges that are not grouped by ascending target are stable-sorted by target first,
    and the table is sized by the largest in-degree when that exceeds ``K + 1`` (a loader graph whose k differs
    from the backbone's ``nb_neighbours``, or a radius graph): then every edge has a slot and the table is the strict
    form without an overflow column - the table ``radius_graph`` builds for the same edges, so a backbone computes
    the same bits from either.  Indices outside ``[0, N)`` raise ``ValueError`` - the device pass validates every
    entry before it writes anything."""
    _need(edge_index, torch.int64, "edge_index")
    if edge_index.dim() != 2 or int(edge_index.shape[0]) != 2:
        raise ValueError("edge_index must be [2, E]")
    edge_index = edge_index.contiguous()
    dev = edge_index.device
    E = int(edge_index.shape[1])
    first = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    wide = False
    for _ in range(3):
        nbr = torch.empty((N, K), dtype=torch.int32, device=dev)
        ovf = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().gn_edge_index_to_table(_p(edge_index), E, N, K, _p(first), _p(nbr), _p(ovf), _p(err), _st()))
        rc = int(err.item())
        if rc == 0:
            return _finish_table(nbr, None if wide else ovf[:N] if N else ovf, K)
        if rc & 1:
            raise ValueError(f"edge_index holds node indices outside [0, {N})")
        if rc & 2:                               # any order is legal input: group by target, keep the order inside a group
            order = torch.argsort(edge_index[1], stable=True)
            edge_index = edge_index[:, order].contiguous()
        elif rc & 4:                             # in-degree above K + 1: size the table by the graph
            K = int(torch.bincount(edge_index[1], minlength=max(N, 1)).max().item())
            wide = True
    raise RuntimeError("gn_edge_index_to_table: could not build the table")       # pragma: no cover


def ptr_to_batch(ptr: Tensor, N: int) -> Tensor:
    _need(ptr, torch.int32, "ptr")
    batch = torch.empty(max(N, 1), dtype=torch.int32, device=ptr.device)[:N]
    _lib.check(_lib.lib().gn_ptr_to_batch(_p(ptr), int(ptr.shape[0]) - 1, _p(batch), _st()))
    return batch


_STD_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "log10": 4}


def standardize(x: Tensor, programs: Sequence[Sequence[Tuple[str, float]]]) -> Tensor:
    """In-place per-column standardisation of ``x[N, F]`` (``gn_standardize``); ``programs[f]`` = up to three
    ``(op, constant)`` steps with op in add / sub / mul / div / log10."""
    _need(x, torch.float32, "x")
    F = len(programs)
    if int(x.shape[1]) != F:
        raise ValueError("one program per column")
    nops = (ctypes.c_int32 * F)(*[len(p) for p in programs])
    op = (ctypes.c_int32 * (3 * F))()
    cst = (ctypes.c_float * (3 * F))()
    for f, prog in enumerate(programs):
        if len(prog) > 3:
            raise ValueError("at most 3 steps per column")
        for k, (name, c) in enumerate(prog):
            op[3 * f + k] = _STD_OPS[name]
            cst[3 * f + k] = float(c)
    _lib.check(_lib.lib().gn_standardize(_p(x), _rows(x, "x"), int(x.shape[0]), F, ctypes.cast(nops, ctypes.c_void_p),
                                         ctypes.cast(op, ctypes.c_void_p), ctypes.cast(cst, ctypes.c_void_p), _st()))
    return x


def graph_globals(x: Tensor, ptr: Tensor, g: NeighbourTable, n_pulses: Tensor) -> Tensor:
    _need(x, torch.float32, "x"); _need(n_pulses, torch.int32, "n_pulses")
    B, F = int(ptr.shape[0]) - 1, int(x.shape[1])
    if F > 32:
        # the kernel sums up to 32 columns (RNN_TITO feeds 69): column blocks of 32, the last one moved left so that it
        # is full.  A column's mean does not depend on its block; the homophily and log10(n) columns come from block 0.
        first = graph_globals(x[:, :32], ptr, g, n_pulses)
        means = [first[:, :32]]
        for c0 in range(32, F, 32):
            lo = min(c0, F - 32)
            means.append(graph_globals(x[:, lo:lo + 32], ptr, g, n_pulses)[:, c0 - lo:32])
        return torch.cat(means + [first[:, 32:]], dim=1)
    out = torch.empty((B, F + 5), dtype=torch.float32, device=x.device)
    N = int(x.shape[0])
    scratch = _event_scratch(B, N, 0, x.device)         # a few huge events: one workgroup per event slice
    with _timed("graph_globals"):
        _lib.check(_lib.lib().gn_graph_globals_ws(_p(x), _rows(x, "x"), F, _p(ptr), B, N, _p(g.nbr), _p(g.ovf), g.K,
                                                  _p(n_pulses), _p(out), _p(scratch), _st()))
    return out


def _event_scratch(B: int, N: int, C: int, device) -> Optional[Tensor]:
    """Scratch of the per-event reductions for a batch of a few huge events (None: one workgroup per event; same result)."""
    nbytes = int(_lib.lib().gn_event_scratch_bytes(B, N, C))
    if B < 1 or B > 64 or N <= 1024 or nbytes <= 0:
        return None
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def concat_globals(x: Tensor, gv: Optional[Tensor], batch: Tensor, ld0: int,
                   dtype: torch.dtype = torch.float32) -> Tensor:
    """``[x | gv[batch] | 0]`` with row pitch ``ld0`` (a multiple of 32), as fp32 or bf16."""
    N, F = int(x.shape[0]), int(x.shape[1])
    G = 0 if gv is None else int(gv.shape[1])
    x0 = torch.empty((N, ld0), dtype=dtype, device=x.device)
    gvt = gv if gv is not None else x
    _lib.check(_lib.lib().gn_concat_globals(_p(x), _rows(x, "x"), F, _p(gvt), G, _p(batch), N, _p(x0), ld0,
                                            int(dtype == torch.bfloat16), _st()))
    return x0


# ------------------------------------------------------------------------------ dense layers
Seg = Tuple[Tensor, int]   # (fp32 or bf16 tensor [M, >=width] with unit column stride, kernel-side width)


def act_dtype(mode: int) -> torch.dtype:
    """Storage type of activations / activation gradients between kernels (``include/graphnet_amd.h``)."""
    return mode_dtype(mode)


def seg_unit(dtype: torch.dtype) -> int:
    """Granularity of a segment's kernel-side width: one 16-byte load (4 floats / 8 bf16)."""
    return 8 if dtype == torch.bfloat16 else 4


def gemm_kunit(mode: int) -> int:
    """K padding unit of the per-node GEMM operands: bf16 uses 64-deep LDS blocks."""
    return 64 if mode == MODE_BF16 else 32


def _seg_arrays(segs: Sequence[Seg], with_kpad: bool, kunit: int = 32):
    n = len(segs)
    ptrs = (ctypes.c_void_p * n)(*[s[0].data_ptr() for s in segs])
    lds = (ctypes.c_int64 * n)(*[_rows(s[0], "segment") for s in segs])
    widths = (ctypes.c_int32 * n)(*[int(s[1]) for s in segs])
    kpads = (ctypes.c_int32 * n)(*[round_up(int(s[1]), kunit) for s in segs]) if with_kpad else None
    dt = segs[0][0].dtype
    for s in segs:
        _need(s[0], dt, "segment")
    if dt not in (torch.float32, torch.bfloat16):
        raise TypeError("segments must be fp32 or bf16")
    return n, ptrs, lds, widths, kpads, int(dt == torch.bfloat16)


def pack_weight(W: Tensor, seg_widths: Sequence[int], dtype: torch.dtype, kunit: int = 32) -> Tensor:
    """``W[N, sum widths]`` fp32 -> ``[ceil128(N)][sum ceil_kunit(width)]`` of ``dtype`` (zero padded).
    ``kunit`` = 32 for the EdgeConv kernels' operands, :func:`gemm_kunit` for :func:`linear_fwd`."""
    N = int(W.shape[0])
    parts, off = [], 0
    for w in seg_widths:
        blk = W[:, off:off + w]
        parts.append(torch.nn.functional.pad(blk, (0, round_up(w, kunit) - w)))
        off += w
    Wp = torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]
    Wp = torch.nn.functional.pad(Wp, (0, 0, 0, round_up(N, 128) - N))
    return Wp.to(dtype).contiguous()


def pack_weights(desc: Tensor) -> None:
    """Replay a recorded list of weight-operand copies (``gn_pack_weights``; ``desc`` int64 ``[n, 10]``)."""
    _need(desc, torch.int64, "desc")
    _lib.check(_lib.lib().gn_pack_weights(_p(desc), int(desc.shape[0]), _st()))


def linear_fwd(mode: int, segs: Sequence[Seg], Wp: Tensor, n_real: int, bias: Optional[Tensor] = None,
               relu: bool = False, gate: Optional[Tensor] = None, out: Optional[Tensor] = None,
               accum: bool = False, out_lowp: bool = False, out_cols: Optional[int] = None) -> Tensor:
    """``out[M, n_real] = epi(cat(segs) @ W^T + bias)`` on MFMA.  ``Wp`` from
    ``pack_weight(W, widths, dtype, kunit=gemm_kunit(mode))``."""
    n, ptrs, lds, widths, kpads, a_lowp = _seg_arrays(segs, True, gemm_kunit(mode))
    M = int(segs[0][0].shape[0])
    Npad, Kp = int(Wp.shape[0]), int(Wp.shape[1])
    if out is None:
        cols = out_cols if out_cols is not None else n_real
        out = torch.empty((M, cols), dtype=mode_dtype(mode) if out_lowp else torch.float32, device=Wp.device)
        if cols > n_real:
            out[:, n_real:].zero_()
    with _timed("linear_fwd", f"linear_fwd[{sum(int(s[1]) for s in segs)}x{n_real}]"):
        _lib.check(_lib.lib().gn_linear_fwd(
            mode, n, ctypes.cast(ptrs, ctypes.c_void_p), a_lowp, ctypes.cast(lds, ctypes.c_void_p),
            ctypes.cast(widths, ctypes.c_void_p), ctypes.cast(kpads, ctypes.c_void_p), M, _p(Wp), Kp, Npad, n_real,
            _p(bias), _p(gate), int(gate is not None and gate.dtype == torch.bfloat16),
            0 if gate is None else _rows(gate, "gate"), int(relu), int(accum),
            _p(out), _rows(out, "out"), int(out.dtype == torch.bfloat16), _st()))
    return out


def linear_wgrad(mode: int, dY: Tensor, n1: int, segs: Sequence[Seg], out: Optional[Tensor] = None,
                 accum: bool = False, with_bias: bool = False):
    """``dW[n1, sum widths] (+)= dY[:, :n1]^T @ cat(segs)`` (deterministic split reduction).
    ``with_bias``: also return ``db[n1] = colsum(dY)`` from the same pass -> ``(dW, db)``."""
    n, ptrs, lds, widths, _, x_lowp = _seg_arrays(segs, False)
    M = int(dY.shape[0])
    ktot = sum(int(s[1]) for s in segs)
    L = _lib.lib()
    parts = int(L.gn_linear_wgrad_parts(mode, M, n1, n, ctypes.cast(widths, ctypes.c_void_p)))
    dev = dY.device
    slab = torch.empty(parts * n1 * ktot, dtype=torch.float32, device=dev)
    db = dbp = None
    if with_bias:
        dbp = torch.empty(max(parts, int(L.gn_colsum_blocks(M))) * n1, dtype=torch.float32, device=dev)
        db = torch.empty(n1, dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty((n1, ktot), dtype=torch.float32, device=dev)
    with _timed("linear_wgrad", f"linear_wgrad[{ktot}x{n1}]"):
        _lib.check(L.gn_linear_wgrad(mode, _p(dY), int(dY.dtype == torch.bfloat16), _rows(dY, "dY"), n1, n,
                                     ctypes.cast(ptrs, ctypes.c_void_p), x_lowp,
                                     ctypes.cast(lds, ctypes.c_void_p), ctypes.cast(widths, ctypes.c_void_p), M,
                                     _p(slab), _p(dbp), _p(out), _p(db), int(accum), _st()))
    return (out, db) if with_bias else out


def colsum(X: Tensor, C: int, out: Optional[Tensor] = None, accum: bool = False) -> Tensor:
    _need(X, torch.float32, "X")
    L = _lib.lib()
    M = int(X.shape[0])
    part = torch.empty(int(L.gn_colsum_blocks(M)) * C, dtype=torch.float32, device=X.device)
    if out is None:
        out = torch.empty(C, dtype=torch.float32, device=X.device)
    with _timed("colsum"):
        _lib.check(L.gn_colsum(_p(X), _rows(X, "X"), M, C, _p(part), _p(out), int(accum), _st()))
    return out


# ------------------------------------------------------------------------------ EdgeConv
def _edge_entry(which: str, act: str):
    """(C entry, timer tag) of the edge-convolution pass ``which`` for the edge MLP's activation."""
    if act == "relu":
        return getattr(_lib.lib(), f"gn_edgeconv_{which}"), ""
    if act == "leaky_relu":
        return getattr(_lib.lib(), f"gn_edgeconv_leaky_{which}"), "leaky_"
    raise ValueError(f"fused edge convolution: activation {act!r} (relu or leaky_relu)")


def edgeconv_leaky_supported(mode: int, g: NeighbourTable, H1p: int, H1: int, H2: int) -> bool:
    """Whether the leaky-relu edge convolution of this shape runs on the persistent kernels (else: the tiled ones)."""
    return bool(_lib.lib().gn_edgeconv_leaky_supported(mode, g.K, H1p, H1, H2))


EDGE_PLAN_FIELDS = ("supported", "persistent", "variant", "ovf", "compact_shape", "compact_model", "shape_persistent", "fwd_ws")


def edgeconv_plan(mode: int, g: NeighbourTable, H1p: int, H1: int, H2: int, act: str = "relu") -> dict:
    """Which kernels the passes of this layer run (``gn_edgeconv_plan``: the dispatch rule's own answer under this
    process's ``GN_*`` switches; host only).  Keys: :data:`EDGE_PLAN_FIELDS` - ``persistent``: table rows on the persistent
    bf16 kernels (else the tiled ones); ``ovf``: 0 no overflow list, 1 tiled overflow-row kernels, 2 the GEMM path;
    ``compact_shape``: :func:`edgeconv_bwd_gather_compact` takes the layer; ``fwd_ws``: wave-specialised forward."""
    out = (ctypes.c_int32 * 8)()
    _lib.lib().gn_edgeconv_plan(mode, g.K, g.N, H1p, H1, H2, {"relu": 0, "leaky_relu": 2}[act], int(g.ovf_cnt is not None),
                                ctypes.cast(out, ctypes.c_void_p))
    return dict(zip(EDGE_PLAN_FIELDS, (int(v) for v in out)))


def edgeconv_fwd(mode: int, g: NeighbourTable, PQ: Tensor, H1p: int, W2p: Tensor, b2: Tensor, H2: int,
                 out: Optional[Tensor] = None, coord_cols: Optional[Sequence[int]] = None, H1: Optional[int] = None,
                 act: str = "relu"):
    """``out[i] = sum_j act(act(P[i]+Q[j]) W2^T + b2)``, ``act``: "relu" (DynEdge) or "leaky_relu" (DynEdgeJINST:
    ``gn_edgeconv_leaky_*``, pass the same ``act`` and ``H1`` to :func:`edgeconv_dw2` and :func:`edgeconv_bwd`);
    ``H1`` (default ``H1p``) is the real hidden width:
    columns ``H1..H1p-1`` of P, Q and W2p are the packed layout's zero padding.  Returns (out [N,H2] in the mode's activation
    type, relu bit mask) or, with ``coord_cols`` (<= 8 output columns), (out, mask, coords fp32 [N, 8])
    where ``coords[:, d]`` is the fp32 value of column ``coord_cols[d]`` (next layer's k-NN input)."""
    _need(PQ, mode_dtype(mode), "PQ"); _need(W2p, mode_dtype(mode), "W2p"); _need(b2, torch.float32, "b2")
    N = g.N
    if out is None:
        out = torch.empty((N, H2), dtype=act_dtype(mode), device=PQ.device)
    _need(out, act_dtype(mode), "out")
    nbytes = int(_lib.lib().gn_edgeconv_saved_bytes(N, g.K, H1p, H2))
    mask = torch.empty(nbytes, dtype=torch.uint8, device=PQ.device)     # opaque saved-for-backward buffer
    coords, cc, nc = None, None, 0
    if coord_cols is not None:
        nc = len(coord_cols)
        if nc > 8:
            raise ValueError("at most 8 coordinate columns")
        coords = torch.zeros((max(N, 1), 8), dtype=torch.float32, device=PQ.device)
        cc = (ctypes.c_int32 * max(nc, 1))(*[int(c) for c in coord_cols])
    entry, tag = _edge_entry("fwd", act)
    with _timed("edgeconv_fwd", f"edgeconv_{tag}fwd[{H1p}x{H2}]"):
        _lib.check(entry(mode, *g.c_args(), _p(PQ), H1p, H1p if H1 is None else int(H1), _p(W2p), _p(b2), H2, _p(out),
                         _rows(out, "out"), _p(coords), None if cc is None else ctypes.cast(cc, ctypes.c_void_p), nc,
                         _p(mask), _st()))
    if coord_cols is not None:
        return out, mask, coords[:N]
    return out, mask


def edgeconv_bwd(mode: int, g: NeighbourTable, PQ: Tensor, H1p: int, H2: int, gout: Tensor, mask: Tensor,
                 W2Tp: Tensor, dpre: Tensor, dP: Tensor, act: str = "relu", H1: Optional[int] = None) -> None:
    _need(gout, act_dtype(mode), "gout"); _need(dP, act_dtype(mode), "dP")
    entry, tag = _edge_entry("bwd", act)
    width = () if act == "relu" else (H1p if H1 is None else int(H1),)       # the leaky entry also takes the real width
    with _timed("edgeconv_bwd", f"edgeconv_{tag}bwd[{H1p}x{H2}]"):
        _lib.check(entry(mode, *g.c_args(), _p(PQ), H1p, *width, H2, _p(gout), _rows(gout, "gout"),
                         _p(mask), _p(W2Tp), int(W2Tp.shape[1]), _p(dpre), _p(dP), _rows(dP, "dP"), _st()))


def edgeconv_dw2(mode: int, g: NeighbourTable, PQ: Tensor, H1p: int, H1: int, H2: int, gout: Tensor,
                 mask: Tensor, act: str = "relu") -> Tuple[Tensor, Tensor]:
    """Returns (dW2 [H2, H1], db2 [H2]).  Must run before :func:`edgeconv_bwd` of the same layer."""
    L = _lib.lib()
    _need(gout, act_dtype(mode), "gout")
    nslab = int(L.gn_edgeconv_dw2_slabs(mode, g.N, g.K, H1p, H2))
    dev = PQ.device
    slab = torch.empty(nslab * H2 * H1, dtype=torch.float32, device=dev)
    bpart = torch.empty(nslab * H2, dtype=torch.float32, device=dev)
    entry, tag = _edge_entry("dw2", act)
    with _timed("edgeconv_dw2", f"edgeconv_{tag}dw2[{H1p}x{H2}]"):
        _lib.check(entry(mode, *g.c_args(), _p(PQ), H1p, H1, H2, _p(gout), _rows(gout, "gout"), _p(mask),
                         _p(slab), _p(bpart), _st()))
    dW2 = torch.empty((H2, H1), dtype=torch.float32, device=dev)
    db2 = torch.empty(H2, dtype=torch.float32, device=dev)
    with _timed("reduce_slabs"):
        _lib.check(L.gn_edgeconv_dw2_reduce(mode, _p(g.ovf_cnt), g.N, g.K, H1p, H1, H2, int(act == "leaky_relu"), _p(slab),
                                            _p(bpart), _p(dW2), _p(db2), _st()))
    return dW2, db2


def dpre_compact_supported(mode: int, g: NeighbourTable, H1p: int, H1: int, H2: int) -> bool:
    """Whether the backward of this layer can keep ``dpre`` compact (``gn_edgeconv_dpre_compact_supported``: bf16 mode, the
    persistent-kernel shapes) AND the path is switched on (``GN_DPRE_COMPACT=1``: opt-in, it measured slower than the dense
    pair - DESIGN.md 7h)."""
    return bool(_lib.lib().gn_edgeconv_dpre_compact_supported(mode, g.K, H1p, H1, H2))


def edgeconv_bwd_gather_compact(g: NeighbourTable, PQ: Tensor, H1p: int, H1: int, H2: int, gout: Tensor, mask: Tensor,
                                W2Tp: Tensor, dPQ: Tensor) -> None:
    """``dPQ[:, :H1p]`` (dP) and ``dPQ[:, H1p:]`` (dQ) of one layer with the edge-row tensor ``dpre`` kept COMPACT between the
    backward kernel and the source gather: the elements whose h-bit is clear (about half) are never written or read
    (``csrc/dpre_compact.hip``).  Same values, same summation order as :func:`edgeconv_bwd` + :func:`edgeconv_dq_gather`:
    bit-identical results.  Must run after :func:`edgeconv_dw2` of the layer (which writes the h-bits)."""
    L = _lib.lib()
    _need(gout, torch.bfloat16, "gout"); _need(dPQ, torch.bfloat16, "dPQ"); _need(PQ, torch.bfloat16, "PQ")
    dev = PQ.device
    g.build_reverse()
    plan = torch.empty(int(L.gn_edgeconv_dpre_plan_bytes(g.N, g.K)), dtype=torch.uint8, device=dev)
    dpre_c = torch.empty(int(L.gn_edgeconv_dpre_compact_bytes(g.N, g.K, H1p)), dtype=torch.uint8, device=dev)
    dpre_ovf = torch.empty((max(g.N, 1), H1p), dtype=torch.bfloat16, device=dev) if g.ovf_cnt is not None else None
    with _timed("dpre_plan"):
        _lib.check(L.gn_edgeconv_dpre_plan(g.N, g.K, H1p, H1, H2, _p(mask), _p(plan), _st()))
    dP, dQ = dPQ[:, :H1p], dPQ[:, H1p:]
    with _timed("edgeconv_bwd", f"edgeconv_bwd[{H1p}x{H2}]"):
        _lib.check(L.gn_edgeconv_bwd_compact(*g.c_args(), _p(PQ), H1p, H1, H2, _p(gout), _rows(gout, "gout"), _p(mask), _p(W2Tp),
                                             int(W2Tp.shape[1]), _p(plan), _p(dpre_c), _p(dpre_ovf), _p(dP), _rows(dP, "dP"), _st()))
    with _timed("edgeconv_dq_gather"):
        _lib.check(L.gn_edgeconv_dq_gather_compact(g.N, g.K, H1p, H1, H2, _p(mask), _p(plan), _p(dpre_c), _p(dpre_ovf),
                                                   _p(g.rev_ptr), _p(g.rev_rows), _p(g.rev_hubs), _p(g.rev_nhubs), _p(dQ),
                                                   _rows(dQ, "dQ"), _st()))


def edgeconv_dq_gather(mode: int, g: NeighbourTable, dpre: Tensor, H1p: int, dQ: Tensor) -> None:
    g.build_reverse()
    _need(dQ, act_dtype(mode), "dQ")
    with _timed("edgeconv_dq_gather"):
        _lib.check(_lib.lib().gn_edgeconv_dq_gather(mode, _p(dpre), H1p, _p(g.rev_ptr), _p(g.rev_rows),
                                                    _p(g.rev_hubs), _p(g.rev_nhubs), g.N, _p(dQ),
                                                    _rows(dQ, "dQ"), _st()))


# ------------------------------------------------------------------------------ EdgeConvTito (leaky relu, max), fused
def edgeconv_max_supported(mode: int, g: NeighbourTable, H1p: int, H2: int) -> bool:
    """Whether the fused EdgeConvTito kernels take this layer (bf16, no overflow rows, K <= 16, H1p = H2 = 256)."""
    return g.ovf is None and bool(_lib.lib().gn_edgeconv_max_supported(mode, g.K, H1p, H2))


def exact_table(g: NeighbourTable) -> NeighbourTable:
    """The same graph as a table WITHOUT overflow rows: the (k+1)-th neighbours become column K (static graphs of
    DynEdgeTITO: built once per batch, shared by all DynTrans layers)."""
    if g.ovf is None:
        return g
    nbr = torch.cat([g.nbr, g.ovf.reshape(-1, 1)], dim=1).contiguous()
    t = NeighbourTable(nbr, None, None, None, None, g.K + 1)
    ev = getattr(g, "event_ptr", None)
    if ev is not None:
        t.event_ptr = ev
    return t


def edgeconv_max_fwd(g: NeighbourTable, PQ: Tensor, H1p: int, W2p: Tensor, b2: Tensor, H2: int):
    """``out[i] = leaky(max_j (leaky(P[i] + Q[j]) W2^T + b2))`` -> (out bf16 [N, H2], saved)."""
    _need(PQ, torch.bfloat16, "PQ"); _need(W2p, torch.bfloat16, "W2p"); _need(b2, torch.float32, "b2")
    N = g.N
    out = torch.empty((N, H2), dtype=torch.bfloat16, device=PQ.device)
    saved = torch.empty(int(_lib.lib().gn_edgeconv_saved_bytes(N, g.K, H1p, H2)), dtype=torch.uint8, device=PQ.device)
    with _timed("edgeconv_fwd", f"edgeconv_max_fwd[{H1p}x{H2}]"):
        _lib.check(_lib.lib().gn_edgeconv_max_fwd(_p(g.nbr), N, g.K, _p(PQ), H1p, _p(W2p), _p(b2), H2, _p(out),
                                                  _rows(out, "out"), _p(saved), _st()))
    return out, saved


def edgeconv_max_arg_rank(g: NeighbourTable, saved: Tensor, H1p: int, H2: int) -> Tensor:
    """Which neighbour supplied the maximum of every (centre, column) in :func:`edgeconv_max_fwd`: int32 ``[N, H2]``, the
    edge's rank in the centre's neighbour list (= table column), -1 where the centre has no edge.  Read from the one-hot
    slot masks in ``saved`` (tests / traces: the routing decision of the max aggregation, for teacher forcing)."""
    offs = (ctypes.c_int64 * 3)()
    _lib.lib().gn_edgeconv_saved_offsets(g.N, g.K, H1p, H2, ctypes.cast(offs, ctypes.c_void_p))
    S = g.S
    nbytes = g.N * H2 * (2 if S > 8 else 1)
    raw = saved[int(offs[1]): int(offs[1]) + nbytes]
    m = (raw.view(torch.int16).to(torch.int32) & 0xFFFF) if S > 8 else raw.to(torch.int32)
    m = m.reshape(g.N, H2)
    rank = torch.full_like(m, -1)
    for b in range(S):
        rank = torch.where((m >> b) & 1 == 1, torch.full_like(m, b), rank)
    return rank


def argrow_to_rank(g: NeighbourTable, argrow: Tensor, C: int) -> Tensor:
    """:func:`slot_reduce`'s arg rows (edge-row ids, -1 = none) as ranks in the centre's neighbour list: table slot s ->
    s, overflow row (the (k+1)-th neighbour) -> K."""
    r = argrow.reshape(g.N, C)
    S, main = g.S, g.N * g.S
    return torch.where(r < 0, r, torch.where(r < main, r % S, torch.full_like(r, g.K)))


def edgeconv_max_dw2(g: NeighbourTable, PQ: Tensor, H1p: int, H1: int, H2: int, gout: Tensor, saved: Tensor):
    """(dW2 [H2, H1], db2 [H2]); ``gout`` = d(loss)/d(out) * leaky'(out), bf16.  Must run before :func:`edgeconv_max_bwd`."""
    L = _lib.lib()
    _need(gout, torch.bfloat16, "gout")
    nslab = int(L.gn_edgeconv_max_dw2_slabs(g.N, g.K, H1p))
    dev = PQ.device
    slab = torch.empty(nslab * H2 * H1, dtype=torch.float32, device=dev)
    bpart = torch.empty(nslab * H2, dtype=torch.float32, device=dev)
    with _timed("edgeconv_dw2", f"edgeconv_max_dw2[{H1p}x{H2}]"):
        _lib.check(L.gn_edgeconv_max_dw2(_p(g.nbr), g.N, g.K, _p(PQ), H1p, H1, H2, _p(gout), _rows(gout, "gout"), _p(saved),
                                         _p(slab), _p(bpart), _st()))
    dW2 = torch.empty((H2, H1), dtype=torch.float32, device=dev)
    db2 = torch.empty(H2, dtype=torch.float32, device=dev)
    with _timed("reduce_slabs"):
        _lib.check(L.gn_reduce_slabs(_p(slab), nslab, H2 * H1, _p(dW2), 0, _st()))
        _lib.check(L.gn_reduce_slabs(_p(bpart), nslab, H2, _p(db2), 0, _st()))
    return dW2, db2


def edgeconv_max_bwd(g: NeighbourTable, H1p: int, H2: int, gout: Tensor, saved: Tensor, W2Tp: Tensor, dpre: Tensor,
                     dP: Tensor) -> None:
    _need(gout, torch.bfloat16, "gout"); _need(dP, torch.bfloat16, "dP"); _need(dpre, torch.bfloat16, "dpre")
    with _timed("edgeconv_bwd", f"edgeconv_max_bwd[{H1p}x{H2}]"):
        _lib.check(_lib.lib().gn_edgeconv_max_bwd(_p(g.nbr), g.N, g.K, H1p, H2, _p(gout), _rows(gout, "gout"), _p(saved),
                                                  _p(W2Tp), int(W2Tp.shape[1]), _p(dpre), _p(dP), _rows(dP, "dP"), _st()))


# ------------------------------------------------------------------------------ unfused variant blocks
ACT_CODES = {"relu": 0, "gelu": 1, "leaky_relu": 2, "identity": 3}


def edge_rows(g: NeighbourTable) -> Tuple[Tensor, Tensor]:
    """(ic, jc): centre / source of every edge row of ``g`` (jc = -1 for empty slots); cached on the table."""
    cached = getattr(g, "_rows_cache", None)
    if cached is not None:
        return cached
    dev = g.nbr.device
    ic = torch.empty(g.rows, dtype=torch.int32, device=dev)
    jc = torch.empty(g.rows, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().gn_edge_rows(*g.c_args(), _p(ic), _p(jc), _st()))
    g._rows_cache = (ic, jc)
    return ic, jc


class CompactRows:
    """The existing edges of a table as rows (``gn_rows_compact``): ``ic`` / ``jc`` [N*K + N] ((0, -1) beyond the last
    edge), ``row_ptr`` [N + 1]; ``rows`` = the capacity N*K + N (the number of edges stays on the device)."""

    def __init__(self, g: NeighbourTable):
        L = _lib.lib()
        dev, N, K = g.nbr.device, g.N, g.K
        self.g = g
        self.rows = max(N * K + N, 1)
        self.ic = torch.empty(self.rows, dtype=torch.int32, device=dev)
        self.jc = torch.empty(self.rows, dtype=torch.int32, device=dev)
        self.row_ptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        deg = torch.empty(max(N, 1), dtype=torch.int32, device=dev)
        tmp = torch.empty(int(L.gn_scan_tmp_ints(max(N, 1))), dtype=torch.int32, device=dev)
        with _timed("generic_edge"):
            _lib.check(L.gn_rows_compact(_p(g.nbr), _p(g.ovf), N, K, _p(deg), _p(tmp), _p(self.row_ptr), _p(self.ic), _p(self.jc),
                                         _st()))
        self._rev = None

    def sum(self, m: Tensor, C: int) -> Tensor:
        """out[i] = sum of centre i's rows of ``m`` (``gn_segment_rows_sum``): ``slot_sum`` on the compact rows."""
        if m.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("m must be fp32 or bf16")
        _need(m, m.dtype, "m")
        out = torch.empty((self.g.N, C), dtype=torch.float32, device=m.device)
        with _timed("generic_edge"):
            _lib.check(_lib.lib().gn_segment_rows_sum(_p(m), _rows(m, "m"), C, self.g.N, _p(self.row_ptr), _p(out), C,
                                                      1 if m.dtype == torch.bfloat16 else 0, _st()))
        return out

    def reverse_view(self) -> NeighbourTable:
        """The table with its reverse lists rewritten in compact row ids (for ``edgeconv_dq_gather`` on compact rows)."""
        if self._rev is None:
            import copy
            g = self.g
            g.build_reverse()
            out = torch.empty_like(g.rev_rows)
            with _timed("rev_build"):
                _lib.check(_lib.lib().gn_rev_rows_compact(_p(g.nbr), _p(g.ovf_centre), g.N, g.K, _p(self.row_ptr), _p(g.rev_ptr),
                                                          _p(g.rev_rows), _p(out), _st()))
            v = copy.copy(g)
            v.rev_rows = out
            self._rev = v
        return self._rev


def compact_rows(g: NeighbourTable) -> CompactRows:
    cached = getattr(g, "_compact_cache", None)
    if cached is None:
        cached = CompactRows(g)
        g._compact_cache = cached
    return cached


def edge_gather_pre(PQ: Tensor, H1p: int, ic: Tensor, jc: Tensor, act: str = "identity", lowp: bool = False) -> Tensor:
    """Edge rows ``act(P[ic] + Q[jc])`` (``act``: "identity" or "leaky_relu"), fp32 or bf16 (``lowp``)."""
    _need(PQ, torch.float32, "PQ")
    R = int(ic.shape[0])
    pre = torch.empty((R, H1p), dtype=torch.bfloat16 if lowp else torch.float32, device=PQ.device)
    with _timed("generic_edge"):
        _lib.check(_lib.lib().gn_edge_gather_pre(_p(PQ), H1p, _p(ic), _p(jc), R, ACT_CODES[act], _p(pre), int(lowp), _st()))
    return pre


def rownorm_act_fwd(z: Tensor, C: int, act: str, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None,
                    valid: Optional[Tensor] = None, cpad: Optional[int] = None, eps: float = 1e-5, lowp: str = "no"):
    """``act(LayerNorm(z[:, :C]))`` (LayerNorm only with gamma/beta) -> (a [R, cpad] fp32, stats [R, 2] | None).
    ``lowp``: "no" (fp32 result), "only" (bf16 result instead: operands of the MFMA GEMMs that are not needed in
    fp32) or "both" -> ((a fp32, a bf16), stats)."""
    if z.dtype not in (torch.float32, torch.bfloat16):      # bf16: a pre-activation kept in bf16 (bf16 mode, unfused edge MLPs)
        raise TypeError("rownorm_act_fwd: z must be fp32 or bf16")
    _need(z, z.dtype, "z")
    R = int(z.shape[0])
    cpad = C if cpad is None else cpad
    a = torch.empty((R, cpad), dtype=torch.float32, device=z.device) if lowp != "only" else None
    a16 = torch.empty((R, cpad), dtype=torch.bfloat16, device=z.device) if lowp != "no" else None
    stats = torch.empty((R, 2), dtype=torch.float32, device=z.device) if gamma is not None else None
    with _timed("generic_rows"):
        _lib.check(_lib.lib().gn_rownorm_act_fwd(_p(z), _rows(z, "z"), C, _p(valid), _p(gamma), _p(beta), float(eps),
                                                 ACT_CODES[act], _p(a), cpad, cpad, _p(stats), R, _p(a16), cpad,
                                                 1 if z.dtype == torch.bfloat16 else 0, _st()))
    return (a if lowp == "no" else a16 if lowp == "only" else (a, a16)), stats


def rownorm_act_bwd(g: Tensor, z: Tensor, C: int, act: str, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None,
                    stats: Optional[Tensor] = None, valid: Optional[Tensor] = None, gidx: Optional[Tensor] = None,
                    cpad: Optional[int] = None, lowp: str = "no", argrow: Optional[Tensor] = None):
    """Backward of :func:`rownorm_act_fwd` -> (dz [R, cpad], dgamma | None, dbeta | None); ``lowp`` as there
    ("only": dz is bf16, "both": dz is the pair (fp32, bf16)).  ``argrow`` (with ``gidx``): the rows fed a max
    aggregation, ``g`` is routed to the arg rows only.  ``z`` may be a bf16 activation OUTPUT when the activation
    preserves the sign (leaky relu without LayerNorm)."""
    if g.dtype not in (torch.float32, torch.bfloat16) or z.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("g and z must be fp32 or bf16")
    _need(g, g.dtype, "g")
    R = int(z.shape[0])
    cpad = C if cpad is None else cpad
    dz = torch.empty((R, cpad), dtype=torch.float32, device=z.device) if lowp != "only" else None
    dz16 = torch.empty((R, cpad), dtype=torch.bfloat16, device=z.device) if lowp != "no" else None
    t1 = t2 = None
    if gamma is not None:
        if C % 4:
            raise NotImplementedError("LayerNorm widths must be multiples of 4 on the HIP path")
        nblk = max(int(_lib.lib().gn_rownorm_bwd_blocks(R)), 1)       # one partial row per workgroup
        t1 = torch.empty((nblk, C), dtype=torch.float32, device=z.device)
        t2 = torch.empty((nblk, C), dtype=torch.float32, device=z.device)
    with _timed("generic_rows"):
        _lib.check(_lib.lib().gn_rownorm_act_bwd(_p(g), _rows(g, "g"), _p(gidx), _p(z), _rows(z, "z"), C, _p(valid),
                                                 _p(gamma), _p(beta), _p(stats), ACT_CODES[act], _p(dz), cpad, cpad,
                                                 _p(t1), _p(t2), R, _p(dz16), cpad, _p(argrow),
                                                 int(z.dtype == torch.bfloat16) | (2 if g.dtype == torch.bfloat16 else 0), _st()))
    res = dz if lowp == "no" else dz16 if lowp == "only" else (dz, dz16)
    if gamma is None:
        return res, None, None
    return res, colsum(t2, C), colsum(t1, C)


# BatchNorm1d over edge rows (include/graphnet_amd.h: gn_bn_*)
def bn_stats(z: Tensor, C: int, valid: Optional[Tensor], n_valid: Tensor, eps: float):
    """Training statistics over the valid rows -> (mean [C], rstd [C], var_unbiased [C])."""
    _need(z, torch.float32, "z"); _need(n_valid, torch.int32, "n_valid")
    R, dev = int(z.shape[0]), z.device
    L = _lib.lib()
    part = torch.empty(int(L.gn_bn_blocks(R)) * 2 * C, dtype=torch.float32, device=dev)
    sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
    mean, rstd, varu = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(3))
    with _timed("generic_rows"):
        _lib.check(L.gn_bn_sums(0, 3, _p(z), _rows(z, "z"), R, C, _p(valid), None, 0, None, None, None, None, _p(part),
                                _p(sums), _st()))
        _lib.check(L.gn_bn_finalize(_p(sums), _p(n_valid), C, float(eps), _p(mean), _p(rstd), _p(varu), _st()))
    return mean, rstd, varu


def bn_act_fwd(z: Tensor, C: int, valid: Optional[Tensor], mean: Tensor, rstd: Tensor, gamma: Tensor, beta: Tensor,
               act: str, cpad: Optional[int] = None, lowp: bool = False) -> Tensor:
    _need(z, torch.float32, "z")
    R = int(z.shape[0])
    cpad = C if cpad is None else cpad
    a = torch.empty((R, cpad), dtype=torch.bfloat16 if lowp else torch.float32, device=z.device)
    with _timed("generic_rows"):
        _lib.check(_lib.lib().gn_bn_act_fwd(_p(z), _rows(z, "z"), R, C, _p(valid), _p(mean), _p(rstd), _p(gamma), _p(beta),
                                            ACT_CODES[act], _p(a), cpad, cpad, int(lowp), _st()))
    return a


def bn_act_bwd(g: Tensor, z: Tensor, C: int, valid: Optional[Tensor], mean: Tensor, rstd: Tensor, gamma: Tensor,
               beta: Tensor, act: str, n_valid: Optional[Tensor], training: bool = True, cpad: Optional[int] = None,
               lowp: bool = False):
    """-> (dz [R, cpad], dgamma [C], dbeta [C]); ``training=False``: statistics were constants (running stats)."""
    _need(g, torch.float32, "g"); _need(z, torch.float32, "z")
    R, dev = int(z.shape[0]), z.device
    cpad = C if cpad is None else cpad
    L = _lib.lib()
    part = torch.empty(int(L.gn_bn_blocks(R)) * 2 * C, dtype=torch.float32, device=dev)
    sums = torch.empty(2 * C, dtype=torch.float32, device=dev)
    dz = torch.empty((R, cpad), dtype=torch.bfloat16 if lowp else torch.float32, device=dev)
    with _timed("generic_rows"):
        _lib.check(L.gn_bn_sums(1, ACT_CODES[act], _p(z), _rows(z, "z"), R, C, _p(valid), _p(g), _rows(g, "g"), _p(mean),
                                _p(rstd), _p(gamma), _p(beta), _p(part), _p(sums), _st()))
        _lib.check(L.gn_bn_act_bwd(_p(g), _rows(g, "g"), _p(z), _rows(z, "z"), R, C, _p(valid), _p(mean), _p(rstd),
                                   _p(gamma), _p(beta), _p(sums) if training else None, _p(n_valid) if training else None,
                                   ACT_CODES[act], _p(dz), cpad, cpad, int(lowp), _st()))
    return dz, sums[C:], sums[:C]


def slot_sum(m: Tensor, C: int, g: NeighbourTable) -> Tensor:
    _need(m, torch.float32, "m")
    out = torch.empty((g.N, C), dtype=torch.float32, device=m.device)
    with _timed("generic_edge"):
        _lib.check(_lib.lib().gn_slot_sum(_p(m), _rows(m, "m"), C, *g.c_args(), _p(out), C, _st()))
    return out


AGGR_CODES = {"add": 0, "sum": 0, "mean": 1, "max": 2}


def slot_reduce(m: Tensor, C: int, g: NeighbourTable, aggr: str, post_act: str = "identity"):
    """Aggregate the edge rows of every centre (add / mean / max) -> (out [N, C], aux for the backward).
    ``post_act="leaky_relu"`` (max only): ``leaky(max_j m_j)`` = ``max_j leaky(m_j)`` with the same arg rows."""
    _need(m, torch.float32, "m")
    ic, jc = edge_rows(g)
    dev = m.device
    out = torch.empty((g.N, C), dtype=torch.float32, device=dev)
    ovf_row = torch.empty(max(g.N, 1), dtype=torch.int32, device=dev)
    deg = torch.empty(max(g.N, 1), dtype=torch.int32, device=dev)
    code = AGGR_CODES[aggr]
    argrow = torch.empty(max(g.N * C, 1), dtype=torch.int32, device=dev) if code == 2 else None
    with _timed("generic_edge"):
        _lib.check(_lib.lib().gn_slot_reduce(_p(m), _rows(m, "m"), C, *g.c_args(), _p(jc), code, _p(out), C, _p(ovf_row),
                                             _p(deg), _p(argrow), ACT_CODES[post_act], _st()))
    return out, (deg, argrow)


def slot_reduce_bwd(gout: Tensor, C: int, g: NeighbourTable, aggr: str, aux, cpad: Optional[int] = None) -> Tensor:
    """Gradient of :func:`slot_reduce` w.r.t. the edge rows: [rows, cpad] fp32."""
    _need(gout, torch.float32, "gout")
    ic, jc = edge_rows(g)
    cpad = C if cpad is None else cpad
    deg, argrow = aux
    grows = torch.empty((g.rows, cpad), dtype=torch.float32, device=gout.device)
    with _timed("generic_edge"):
        _lib.check(_lib.lib().gn_slot_reduce_bwd(_p(gout), _rows(gout, "gout"), C, _p(ic), _p(jc), g.rows, AGGR_CODES[aggr],
                                                 _p(deg), _p(argrow), _p(grows), cpad, cpad, _st()))
    return grows


# ------------------------------------------------------------------------------ pooling
def _codes(schemes: Sequence[str]):
    return (ctypes.c_int32 * len(schemes))(*[POOL_CODES[s] for s in schemes])


def segment_pool_fwd(x: Tensor, C: int, ptr: Tensor, schemes: Sequence[str], need_arg: bool = True):
    _need(x, torch.float32, "x")
    B = int(ptr.shape[0]) - 1
    out = torch.empty((B, len(schemes) * C), dtype=torch.float32, device=x.device)
    amin = torch.empty((B, C), dtype=torch.int32, device=x.device) if need_arg else None
    amax = torch.empty((B, C), dtype=torch.int32, device=x.device) if need_arg else None
    c = _codes(schemes)
    N = int(x.shape[0])
    scratch = _event_scratch(B, N, C, x.device)
    with _timed("segment_pool_fwd"):
        _lib.check(_lib.lib().gn_segment_pool_fwd_ws(_p(x), _rows(x, "x"), C, _p(ptr), B, N, ctypes.cast(c, ctypes.c_void_p),
                                                     len(schemes), _p(out), _p(amin), _p(amax), _p(scratch), _st()))
    return out, amin, amax


def segment_pool_bwd(gout: Tensor, C: int, ptr: Tensor, batch: Tensor, N: int, schemes: Sequence[str],
                     amin: Tensor, amax: Tensor, gate: Optional[Tensor],
                     dtype: torch.dtype = torch.float32) -> Tensor:
    gout = gout.contiguous()
    _need(gout, torch.float32, "gout")
    if gate is not None:
        _need(gate, torch.float32, "gate")
    ldx = round_up(C, 8)                               # 16-byte row pitch for either type; pad columns = 0
    dx = torch.empty((N, ldx), dtype=dtype, device=gout.device)
    if ldx != C:
        dx[:, C:].zero_()
    c = _codes(schemes)
    with _timed("segment_pool_bwd"):
        _lib.check(_lib.lib().gn_segment_pool_bwd(_p(gout), C, _p(ptr), _p(batch), N, ctypes.cast(c, ctypes.c_void_p),
                                                  len(schemes), _p(amin), _p(amax), _p(gate),
                                                  0 if gate is None else _rows(gate, "gate"), _p(dx), ldx,
                                                  int(dtype == torch.bfloat16), _st()))
    return dx if ldx == C else dx[:, :C]


# ------------------------------------------------------------------------------ ragged self attention (DynTrans)
def attention_plan(ptr: Tensor, sort: bool = True) -> Tensor:
    """Tile plan of the attention kernels (``gn_attention_plan``): int32 ``[2B+1]``, events in descending size."""
    _need(ptr, torch.int32, "ptr")
    B = int(ptr.shape[0]) - 1
    plan = torch.empty(2 * B + 1, dtype=torch.int32, device=ptr.device)
    _lib.check(_lib.lib().gn_attention_plan(_p(ptr), B, _p(plan), int(sort), _st()))
    return plan


def attention_lowp(mode: int, d_model: int, n_head: int) -> bool:
    """bf16 tensors + matrix-core kernels are available for head widths 32 and 64 in bf16 mode."""
    return mode == MODE_BF16 and d_model % n_head == 0 and d_model // n_head in (32, 64)


def drop_thresh(p: float) -> int:
    """Dropout rate -> 32-bit threshold of the counter-based keep rule (``include/graphnet_amd.h``: gn_dropout)."""
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout rate must be in [0, 1)")
    return min(int(round(p * 4294967296.0)), 4294967295)


def dropout(x: Tensor, seed: int, thresh: int, res: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``out = (res or 0) + dropout(x)`` with the stateless keep rule; applied to a gradient with the same seed it
    is its own backward.  ``out=x`` works in place."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("x must be fp32 or bf16")
    if res is not None:
        _need(res, torch.float32, "res")
    rows, cols = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32 if res is not None else x.dtype, device=x.device)
    with _timed("dropout"):
        _lib.check(_lib.lib().gn_dropout(_p(x), _rows(x, "x"), int(x.dtype == torch.bfloat16), _p(res),
                                         0 if res is None else _rows(res, "res"), _p(out), _rows(out, "out"),
                                         int(out.dtype == torch.bfloat16), rows, cols, seed & 0xFFFFFFFF, thresh, _st()))
    return out


def attention_fwd(qkv: Tensor, n_head: int, ptr: Tensor, plan: Tensor, drop: Optional[Tuple[int, int]] = None):
    """``softmax(Q K^T / sqrt(dh)) V`` per head, every pulse attending to its own event (``gn_attention_fwd``).
    ``qkv`` ``[N, 3 d]`` (Q | K | V): fp32 -> exact-fp32 kernels, bf16 -> matrix-core kernels (dh 32 / 64);
    ``plan`` from :func:`attention_plan`; ``drop=(seed, thresh)``: dropout on the attention probabilities.
    -> (out [N, d] in qkv's type, lse2 [N, H] fp32)."""
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("qkv must be fp32 or bf16")
    N, d3 = int(qkv.shape[0]), int(qkv.shape[1])
    d = d3 // 3
    if d3 != 3 * d or d % n_head:
        raise ValueError("qkv must be [N, 3*d] with d a multiple of the number of heads")
    B = int(ptr.shape[0]) - 1
    out = torch.empty((N, d), dtype=qkv.dtype, device=qkv.device)
    lse2 = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    with _timed("attention_fwd"):
        _lib.check(_lib.lib().gn_attention_fwd(int(qkv.dtype == torch.bfloat16), _p(qkv), _rows(qkv, "qkv"), n_head,
                                               d // n_head, _p(ptr), _p(plan), B, N, _p(out), d, _p(lse2),
                                               (drop[0] & 0xFFFFFFFF) if drop else 0, drop[1] if drop else 0, _st()))
    return out, lse2


def attention_drop_layout(ptr: Tensor) -> Tuple[Tensor, int]:
    """Where the SAVED dropout decisions of one batch live (``gn_attention_fwd_bits``): ``evoff`` int64 ``[B + 1]`` =
    running sum of ``ceil(n / 32)^2`` tiles per event, and the words per head plane (32 per tile).  One host
    synchronisation per batch (the plane size is an allocation size); every DynTrans layer of the step reuses it."""
    n = (ptr[1:] - ptr[:-1]).to(torch.int64)
    w = (n + 31) // 32
    evoff = torch.zeros(int(ptr.shape[0]), dtype=torch.int64, device=ptr.device)
    torch.cumsum(w * w, 0, out=evoff[1:])
    return evoff, int(evoff[-1].item()) * 32


def attention_fwd_saved(qkv: Tensor, n_head: int, ptr: Tensor, plan: Tensor, drop: Tuple[int, int],
                        layout: Tuple[Tensor, int]):
    """:func:`attention_fwd` with dropout (bf16 tensors) that also stores every keep decision as a bit, in both
    orientations, for :func:`attention_bwd_saved`.  -> (out, lse2, (bits_r, bits_c)); results are bit-identical to
    :func:`attention_fwd` with the same ``drop``."""
    _need(qkv, torch.bfloat16, "qkv")
    N, d3 = int(qkv.shape[0]), int(qkv.shape[1])
    d = d3 // 3
    if d3 != 3 * d or d % n_head:
        raise ValueError("qkv must be [N, 3*d] with d a multiple of the number of heads")
    if not drop or not drop[1]:
        raise ValueError("attention_fwd_saved needs a dropout threshold")
    B = int(ptr.shape[0]) - 1
    evoff, plane = layout
    _need(evoff, torch.int64, "evoff")
    out = torch.empty((N, d), dtype=qkv.dtype, device=qkv.device)
    lse2 = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    bits_r = torch.empty(max(n_head * plane, 1), dtype=torch.int32, device=qkv.device)
    bits_c = torch.empty(max(n_head * plane, 1), dtype=torch.int32, device=qkv.device)
    with _timed("attention_fwd"):
        _lib.check(_lib.lib().gn_attention_fwd_bits(_p(qkv), _rows(qkv, "qkv"), n_head, d // n_head, _p(ptr), _p(plan), B, N,
                                                    _p(out), d, _p(lse2), drop[0] & 0xFFFFFFFF, drop[1], _p(bits_r),
                                                    _p(bits_c), _p(evoff), plane, _st()))
    return out, lse2, (bits_r, bits_c)


def attention_bwd_saved(qkv: Tensor, n_head: int, ptr: Tensor, plan: Tensor, out: Tensor, lse2: Tensor, dout: Tensor,
                        thresh: int, bits: Tuple[Tensor, Tensor], layout: Tuple[Tensor, int]) -> Tensor:
    """Gradient of :func:`attention_fwd_saved` w.r.t. ``qkv``: the keep decisions are read from ``bits``."""
    _need(qkv, torch.bfloat16, "qkv"); _need(dout, qkv.dtype, "dout"); _need(out, qkv.dtype, "out")
    N, d3 = int(qkv.shape[0]), int(qkv.shape[1])
    d = d3 // 3
    B = int(ptr.shape[0]) - 1
    evoff, plane = layout
    dqkv = torch.empty((N, d3), dtype=qkv.dtype, device=qkv.device)
    delta = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    with _timed("attention_bwd"):
        _lib.check(_lib.lib().gn_attention_bwd_bits(_p(qkv), _rows(qkv, "qkv"), n_head, d // n_head, _p(ptr), _p(plan), B, N,
                                                    _p(out), _rows(out, "out"), _p(dout), _rows(dout, "dout"), _p(lse2),
                                                    _p(delta), _p(dqkv), d3, thresh, _p(bits[0]), _p(bits[1]), _p(evoff),
                                                    plane, _st()))
    return dqkv


def attention_bwd(qkv: Tensor, n_head: int, ptr: Tensor, plan: Tensor, out: Tensor, lse2: Tensor, dout: Tensor,
                  drop: Optional[Tuple[int, int]] = None) -> Tensor:
    """Gradient of :func:`attention_fwd` w.r.t. ``qkv`` -> [N, 3 d] in qkv's type (``out`` / ``dout`` likewise)."""
    _need(dout, qkv.dtype, "dout"); _need(out, qkv.dtype, "out")
    N, d3 = int(qkv.shape[0]), int(qkv.shape[1])
    d = d3 // 3
    B = int(ptr.shape[0]) - 1
    dqkv = torch.empty((N, d3), dtype=qkv.dtype, device=qkv.device)
    delta = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    with _timed("attention_bwd"):
        _lib.check(_lib.lib().gn_attention_bwd(int(qkv.dtype == torch.bfloat16), _p(qkv), _rows(qkv, "qkv"), n_head,
                                               d // n_head, _p(ptr), _p(plan), B, N, _p(out), _rows(out, "out"), _p(dout),
                                               _rows(dout, "dout"), _p(lse2), _p(delta), _p(dqkv), d3,
                                               (drop[0] & 0xFFFFFFFF) if drop else 0, drop[1] if drop else 0, _st()))
    return dqkv


# ------------------------------------------------------------------------------ ragged attention + spacetime bias (DeepIce)
def rel_attention_supported(dh: int) -> bool:
    """Head widths of the biased attention kernels (``gn_rel_attention_supported``)."""
    return bool(_lib.lib().gn_rel_attention_supported(int(dh)))


def rel_attention_freq(dh: int, device) -> Tensor:
    """The ``dh / 2`` frequencies of ``SinusoidalPosEmb(dh)``: the fp32 operations of ``rnn.sinusoidal_pos_emb``, on the host."""
    half_dim = dh / 2
    emb = torch.log(torch.tensor([10000.0], dtype=torch.float32)) / half_dim
    return torch.exp(torch.arange(half_dim) * (-emb)).to(device)


def _rel_check(qkv: Tensor, qp: Tensor, xt: Tensor, freq: Tensor, n_head: int) -> Tuple[int, int]:
    for t, name in ((qkv, "qkv"), (qp, "qp"), (xt, "xt"), (freq, "freq")):
        _need(t, torch.float32, name)
    N, d = int(qp.shape[0]), int(qp.shape[1])
    if int(qkv.shape[0]) != N or int(qkv.shape[1]) != 3 * d or d % n_head or int(xt.shape[0]) != N or int(xt.shape[1]) < 4:
        raise ValueError("need qkv [N, 3*d], qp [N, d] with d a multiple of the number of heads, xt [N, >= 4]")
    dh = d // n_head
    if not rel_attention_supported(dh):
        raise NotImplementedError(f"biased ragged attention: head width {dh} is not built (32 is); no fallback")
    if int(freq.numel()) != dh // 2 or not freq.is_contiguous():
        raise ValueError("freq must hold dh / 2 contiguous frequencies")
    return N, d


def rel_attention_fwd(qkv: Tensor, qp: Tensor, xt: Tensor, freq: Tensor, n_head: int, ptr: Tensor, plan: Tensor):
    """Ragged attention with the spacetime bias of ``DeepIce`` recomputed per pair (``gn_rel_attention_fwd``): scores
    ``q k / sqrt(dh) + qp . s_ij``, ``s_ij`` the sinusoidal embedding of the clipped 4-distance of pulses ``i``, ``j`` (columns
    0-3 of ``xt``: x, y, z, time).  fp32.  -> (out ``[N, d]`` = sum_j a_ij v_j, u ``[N, d]`` = sum_j a_ij s_ij, lse2 ``[N, H]``)."""
    N, d = _rel_check(qkv, qp, xt, freq, n_head)
    B = int(ptr.shape[0]) - 1
    out = torch.empty((N, d), dtype=torch.float32, device=qkv.device)
    u = torch.empty((N, d), dtype=torch.float32, device=qkv.device)
    lse2 = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    with _timed("rel_attention_fwd"):
        _lib.check(_lib.lib().gn_rel_attention_fwd(_p(qkv), _rows(qkv, "qkv"), _p(qp), _rows(qp, "qp"), _p(xt), _rows(xt, "xt"),
                                                   _p(freq), n_head, d // n_head, _p(ptr), _p(plan), B, N, _p(out), d, _p(u), d,
                                                   _p(lse2), _st()))
    return out, u, lse2


def rel_attention_bwd(qkv: Tensor, qp: Tensor, xt: Tensor, freq: Tensor, n_head: int, ptr: Tensor, plan: Tensor,
                      out: Tensor, u: Tensor, lse2: Tensor, dout: Tensor, du: Tensor) -> Tuple[Tensor, Tensor]:
    """Gradients of :func:`rel_attention_fwd` -> (dqkv ``[N, 3 d]``, dqp ``[N, d]``); ``xt`` carries none."""
    N, d = _rel_check(qkv, qp, xt, freq, n_head)
    for t, name in ((out, "out"), (u, "u"), (dout, "dout"), (du, "du"), (lse2, "lse2")):
        _need(t, torch.float32, name)
    B = int(ptr.shape[0]) - 1
    dqkv = torch.empty((N, 3 * d), dtype=torch.float32, device=qkv.device)
    dqp = torch.empty((N, d), dtype=torch.float32, device=qkv.device)
    delta = torch.empty((N, n_head), dtype=torch.float32, device=qkv.device)
    with _timed("rel_attention_bwd"):
        _lib.check(_lib.lib().gn_rel_attention_bwd(_p(qkv), _rows(qkv, "qkv"), _p(qp), _rows(qp, "qp"), _p(xt), _rows(xt, "xt"),
                                                   _p(freq), n_head, d // n_head, _p(ptr), _p(plan), B, N, _p(out),
                                                   _rows(out, "out"), _p(u), _rows(u, "u"), _p(dout), _rows(dout, "dout"),
                                                   _p(du), _rows(du, "du"), _p(lse2), _p(delta), _p(dqkv), 3 * d, _p(dqp), d,
                                                   _st()))
    return dqkv, dqp
