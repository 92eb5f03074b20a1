"""``GNN`` plugin base class and the MI355X-native ``DynEdge`` backbone.

Drop-in for ``graphnet.models.gnn.DynEdge`` (reference ``models/gnn/dynedge.py:21-349``,
plugin ABC ``models/gnn/gnn.py:11-35``): identical keyword signature, identical sub-module
names (``_conv_layers.{l}.nn.{0,2}``, ``_post_processing.{0,2}``, ``_readout.{0}``) so that
reference state-dicts load unchanged, identical output.  Everything between ``data.x`` and the
pooled features runs in ``libgraphnet_amd.so`` (one ``torch.autograd.Function`` orchestrating
the kernels); the tiny read-out MLP on ``[B, 1024]`` stays in torch.
"""
from __future__ import annotations

import os

from typing import Any, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import ops
from .graphs import minkowski_record, radial_record
from .model import REFERENCE, Model

GLOBAL_POOLINGS = ("min", "max", "sum", "mean")


class GNN(*((Model, REFERENCE["GNN"]) if REFERENCE else (Model,))):
    """Base class for all core GNN models (``models/gnn/gnn.py:11-35``).  When the reference is importable this class
    also derives from ``graphnet.models.gnn.gnn.GNN``, so a ``graphnet_amd.DynEdge`` passes the reference's
    ``isinstance(backbone, Model)`` check (``models/standard_model.py:64``) and is captured by its config metaclass."""

    def __init__(self, nb_inputs: int, nb_outputs: int) -> None:
        if REFERENCE:
            super().__init__(nb_inputs, nb_outputs)       # -> graphnet.models.gnn.gnn.GNN.__init__ (gnn.py:14-21)
        else:
            super().__init__()
        self._nb_inputs = nb_inputs
        self._nb_outputs = nb_outputs

    @property
    def nb_inputs(self) -> int:
        return self._nb_inputs

    @property
    def nb_outputs(self) -> int:
        return self._nb_outputs

    def forward(self, data: Any) -> Tensor:  # pragma: no cover - abstract
        raise NotImplementedError


class _ConvParams(torch.nn.Module):
    """Holds the edge MLP under the attribute name ``nn`` (PyG ``EdgeConv.nn``) so the
    state-dict keys equal the reference's ``_conv_layers.{l}.nn.{idx}.{weight,bias}``."""

    def __init__(self, mlp: torch.nn.Sequential, nb_neighbors: int, features_subset: Any):
        super().__init__()
        self.nn = mlp
        self.nb_neighbors = nb_neighbors
        self.features_subset = features_subset


def _maybe(data: Any, key: str) -> Any:
    try:
        return data[key] if key in data else None
    except TypeError:
        return getattr(data, key, None)


def _no_radial_record(data: Any, edge_index: Any, who: str) -> None:
    """Only ``DynEdge`` builds the graph that ``RadialEdges`` recorded on a CPU ``Data``; the other backbones take it as
    ``edge_index`` (the edge definition run on a device batch) and must not build k-NN in its place."""
    if edge_index is None and radial_record(data) is not None:
        raise NotImplementedError(
            f"{who}: the batch carries the parameters of RadialEdges but no edge_index, and {who} does not build radius "
            "graphs; apply RadialEdges to the batch on the device (it sets edge_index) or use DynEdge")


def _subset_cols(subset: Union[slice, Sequence[int]], width: int) -> List[int]:
    if isinstance(subset, slice):
        return list(range(width))[subset]
    return [int(c) for c in subset]


def _kw(w: int, unit: int = 4) -> int:
    """Kernel-side width of a segment: one 16-byte load (4 floats / 8 bf16); the pad columns hold zeros."""
    return ops.round_up(w, unit)


def _ksegs(segs: Sequence[Tuple[Tensor, int]]) -> List[Tuple[Tensor, int]]:
    return [(t, _kw(w, ops.seg_unit(t.dtype))) for t, w in segs]


def _unpad_cols(dW: Tensor, widths: Sequence[int], unit: int = 4) -> Tensor:
    """Drop the pad columns of each segment from a weight gradient."""
    if all(w == _kw(w, unit) for w in widths):
        return dW
    parts, off = [], 0
    for w in widths:
        parts.append(dW[:, off: off + w])
        off += _kw(w, unit)
    return torch.cat(parts, dim=1)


class _WeightBuffers:
    """Persistent, zero-initialised buffers holding the packed (padded / transposed / bf16) operand copies of
    the weights.  Only the real block of a buffer is ever written, so pad rows and columns stay zero.

    The first forward (backward) performs its copies one by one and *records* them as descriptors; as long as
    the parameter storages do not move (in-place optimizers), every later forward (backward) replays the whole
    list with ONE ``gn_pack_weights`` launch instead of ~20 small copy kernels."""

    def __init__(self) -> None:
        self._b: dict = {}
        self._tab: dict = {}          # phase -> dict(sig=..., desc=Tensor | None, rec=[...], live=bool)

    def get(self, key, shape, dtype, device) -> Tensor:
        t = self._b.get(key)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device:
            if t is not None:         # a REPLACED buffer leaves dangling pointers in the recorded lists
                for tab in self._tab.values():
                    tab["desc"], tab["rec"], tab["live"] = None, None, False
            t = torch.zeros(shape, dtype=dtype, device=device)
            self._b[key] = t
        return t

    def begin(self, phase: str, sig: tuple) -> None:
        """``sig``: whatever the copy list depends on (mode, parameter storage pointers)."""
        t = self._tab.get(phase)
        if t is not None and t["desc"] is not None and t["sig"] == sig:
            ops.pack_weights(t["desc"])
            t["live"] = True
        else:
            self._tab[phase] = {"sig": sig, "desc": None, "rec": [], "live": False}
        self._phase = phase

    def copy(self, dst: Tensor, src: Tensor, src2: Optional[Tensor] = None) -> None:
        """dst[...] = src (- src2): done by the step's pack launch when live, else now (and recorded)."""
        t = self._tab[self._phase]
        if t["live"]:
            return                    # this step's pack launch already wrote it
        if src2 is None:
            dst.copy_(src)
        else:
            torch.sub(src, src2, out=dst)
        d2, s2 = (dst, src) if dst.dim() == 2 else (dst.unsqueeze(0), src.unsqueeze(0))
        if d2.stride(1) != 1 or (src2 is not None and src2.stride() != src.stride()):
            t["rec"] = None           # not expressible as a descriptor: stay on the copy-by-copy path
            return
        if t["rec"] is not None:
            t["rec"].append([s2.data_ptr(), 0 if src2 is None else src2.data_ptr(), d2.data_ptr(), s2.stride(0),
                             s2.stride(1), d2.stride(0), d2.shape[0], d2.shape[1], int(dst.dtype == torch.bfloat16), 0])

    def end(self, phase: str, device) -> None:
        t = self._tab.get(phase)
        if t is not None and not t["live"] and t["rec"]:
            t["desc"] = torch.tensor(t["rec"], dtype=torch.int64, device=device)
        if t is not None:
            t["live"] = False


def _packed(wb: _WeightBuffers, key, W: Tensor, dtype: torch.dtype, kunit: int = 32, koffs=None, widths=None) -> Tensor:
    """``ops.pack_weight`` layout (``[ceil128(N)][sum ceil_kunit(width)]``) kept in a persistent buffer.
    ``widths``: column segments of W, each padded to ``kunit`` in the packed K axis."""
    N, K = int(W.shape[0]), int(W.shape[1])
    widths = [K] if widths is None else list(widths)
    kp = sum(ops.round_up(w, kunit) for w in widths)
    buf = wb.get(key, (ops.round_up(N, 128), kp), dtype, W.device)
    off = offp = 0
    for w in widths:
        wb.copy(buf[:N, offp: offp + w], W[:, off: off + w])
        off += w
        offp += ops.round_up(w, kunit)
    return buf


class _DynEdgeFunction(torch.autograd.Function):
    """x, graph -> node features after the post-processing MLP (optionally pooled).

    forward/backward only enqueue kernels of the C ABI on the current stream.
    """

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, *params: Tensor) -> Tensor:  # type: ignore[override]
        mode = cfg["mode"]
        dt = ops.mode_dtype(mode)
        ku = ops.gemm_kunit(mode)
        lowp = mode == ops.MODE_BF16
        batch, ptr, g = cfg["batch"], cfg["ptr"], cfg["graph"]
        nconv, npost = cfg["nconv"], cfg["npost"]
        conv_p = [params[4 * l: 4 * l + 4] for l in range(nconv)]
        post_p = [params[4 * nconv + 2 * t: 4 * nconv + 2 * t + 2] for t in range(npost)]
        N, F = int(x.shape[0]), int(x.shape[1])

        gv = cfg["globals"]
        G = 0 if (gv is None or cfg["globals_after"]) else int(gv.shape[1])
        F0 = F + G
        act = ops.act_dtype(mode)                  # activations between kernels: fp32 / bf16 by mode
        x0 = ops.concat_globals(x, gv if G else None, batch, ops.round_up(F0, 32), dtype=act)
        xs: List[Tuple[Tensor, int]] = [(x0, F0)]
        wb: _WeightBuffers = cfg["wbuf"]
        wsig = (mode,) + tuple(p.data_ptr() for p in params)
        wb.begin("fwd", wsig)
        graphs, PQs, masks = [], [], []
        knn_coords: List[Tensor] = []          # fp32 coordinates each re-built graph was computed from
        plan = cfg.get("plan")                  # built with the layer-1 graph, shared by every layer of the batch
        # Second HIP stream: the k-NN of layer l+1 (vector-ALU bound) runs beside the P|Q GEMM of layer l+1 (HBM
        # bound, needs only the features), the reverse adjacency of every graph (needed by the backward only)
        # beside the edge kernel.  Tensors crossing streams are kept alive until the streams have joined.
        side = cfg.get("side_stream")
        main = torch.cuda.current_stream() if side is not None else None
        keep: List[Any] = []
        graph_ready = None
        if side is not None:
            side.wait_stream(main)
            with torch.cuda.stream(side):
                g.build_reverse()
        for l, (W1, b1, W2, b2) in enumerate(conv_p):
            xin, Fin = xs[-1]
            H1, H2 = int(W1.shape[0]), int(W2.shape[0])
            H1p = ops.round_up(H1, 32)
            Wa, Wb = W1[:, :Fin], W1[:, Fin:]
            # packed [P ; Q] weight: rows 0..H1 = Wa - Wb, rows H1p..H1p+H1 = Wb (pads stay zero)
            Wpq = wb.get(("Wpq", l), (ops.round_up(2 * H1p, 128), ops.round_up(Fin, ku)), dt, x.device)
            bpq = wb.get(("bpq", l), (2 * H1p,), torch.float32, x.device)
            wb.copy(Wpq[:H1, :Fin], Wa, Wb)
            wb.copy(Wpq[H1p:H1p + H1, :Fin], Wb)
            wb.copy(bpq[:H1], b1)
            PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), Wpq, 2 * H1p, bias=bpq, out_lowp=lowp)
            W2p = _packed(wb, ("W2p", l), W2, dt)
            if graph_ready is not None:
                main.wait_event(graph_ready)                 # this layer's graph was built on the side stream
                graph_ready = None
            if l + 1 < nconv:
                cols = _subset_cols(cfg["features_subset"], H2)
                if plan is None:
                    plan = ops.knn_plan(ptr, N)               # query-tile plan: once per batch, all layers
                if lowp and len(cols) <= 8:
                    # bf16 activations: the k-NN coordinates leave the kernel as a separate fp32 copy
                    out, mask, coords = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2.contiguous(), H2, coord_cols=cols, H1=H1)
                    if side is not None:
                        keep.append(coords)
                        side.wait_stream(main)
                        with torch.cuda.stream(side):
                            g_next = ops.knn_graph(coords, list(range(len(cols))), batch, ptr, cfg["k"],
                                                   strict=cfg["strict"], plan=plan)
                            graph_ready = side.record_event()
                            g_next.build_reverse()
                    else:
                        g_next = ops.knn_graph(coords, list(range(len(cols))), batch, ptr, cfg["k"],
                                               strict=cfg["strict"], plan=plan)
                    knn_coords.append(coords[:, :len(cols)])
                else:
                    out, mask = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2.contiguous(), H2, H1=H1)
                    src = out.float() if lowp else out
                    g_next = ops.knn_graph(src, cols, batch, ptr, cfg["k"], strict=cfg["strict"], plan=plan)
                    knn_coords.append(src[:, cols])
            else:
                out, mask = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2.contiguous(), H2, H1=H1)
                g_next = None
            graphs.append(g); PQs.append(PQ); masks.append(mask)
            xs.append((out, H2))
            g = g_next
        ys: List[Tuple[Tensor, int]] = []
        segs = xs
        for t, (W, b) in enumerate(post_p):
            # hidden post-MLP layers are activations (bf16 in bf16 mode); the last one feeds pooling: fp32
            y = ops.linear_fwd(mode, _ksegs(segs), _packed(wb, ("post", t), W, dt, ku, widths=[w for _, w in segs]),
                               int(W.shape[0]),
                               bias=b.contiguous(), relu=True, out_lowp=lowp and t + 1 < npost,
                               out_cols=ops.round_up(int(W.shape[0]), 8))
            ys.append((y, int(W.shape[0])))
            segs = [ys[-1]]
        wb.end("fwd", x.device)
        if side is not None:
            main.wait_stream(side)                           # join: everything the side stream produced is complete
        del keep
        y_last, P = ys[-1]
        ctx.cfg, ctx.xs, ctx.graphs, ctx.PQs, ctx.masks, ctx.ys = cfg, xs, graphs, PQs, masks, ys
        ctx.params = params
        ctx.amin = ctx.amax = None
        cfg["trace"] = ({"conv_out": [t.float() for t, _ in xs], "graphs": graphs, "post": y_last[:, :P],
                         "knn_coords": knn_coords}
                        if cfg.get("want_trace") else None)
        if cfg["pools"]:
            pooled, ctx.amin, ctx.amax = ops.segment_pool_fwd(y_last, P, ptr, cfg["pools"])
            return pooled
        return y_last[:, :P] if int(y_last.shape[1]) != P else y_last

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        cfg = ctx.cfg
        mode = cfg["mode"]
        dt = ops.mode_dtype(mode)
        ku = ops.gemm_kunit(mode)
        lowp = mode == ops.MODE_BF16
        batch, ptr = cfg["batch"], cfg["ptr"]
        nconv, npost = cfg["nconv"], cfg["npost"]
        params = ctx.params
        conv_p = [params[4 * l: 4 * l + 4] for l in range(nconv)]
        post_p = [params[4 * nconv + 2 * t: 4 * nconv + 2 * t + 2] for t in range(npost)]
        xs, ys = ctx.xs, ctx.ys
        wb: _WeightBuffers = cfg["wbuf"]
        wb.begin("bwd", (mode,) + tuple(p.data_ptr() for p in params))
        N = int(xs[0][0].shape[0])
        dev = xs[0][0].device
        grads: List[Optional[Tensor]] = [None] * len(params)

        act = ops.act_dtype(mode)
        unit = ops.seg_unit(act)
        y_last, P = ys[-1]
        gout = gout.contiguous().to(torch.float32)
        if cfg["pools"]:
            dZ = ops.segment_pool_bwd(gout, P, ptr, batch, N, cfg["pools"], ctx.amin, ctx.amax, y_last, dtype=act)
        else:
            dZ = (gout * (y_last[:, :P] > 0)).to(act).contiguous()

        # ---- post-processing MLP, last layer first
        seg_pad = [ops.round_up(w, 32) for _, w in xs]
        seg_off = [sum(seg_pad[:i]) for i in range(len(xs))]
        dXcat = None
        for t in reversed(range(npost)):
            W, b = post_p[t]
            Pt = int(W.shape[0])
            in_segs = xs if t == 0 else [ys[t - 1]]
            dWt, dbt = ops.linear_wgrad(mode, dZ, Pt, _ksegs(in_segs), with_bias=True)
            grads[4 * nconv + 2 * t] = _unpad_cols(dWt, [w for _, w in in_segs], unit)
            grads[4 * nconv + 2 * t + 1] = dbt
            if t > 0:
                yprev, Pprev = ys[t - 1]
                dZ = ops.linear_fwd(mode, _ksegs([(dZ, Pt)]), _packed(wb, ("postT", t), W.t(), dt, ku), Pprev, gate=yprev,
                                    out_lowp=lowp, out_cols=ops.round_up(Pprev, 8))
            else:
                # gradient w.r.t. the skip-cat input, segment 0 (the raw pulse features) excluded: nobody reads it
                ncols = sum(seg_pad) - seg_off[1]
                WT = wb.get(("catT",), (ops.round_up(ncols, 128), ops.round_up(Pt, ku)), dt, dev)
                off = xs[0][1]
                for s_ in range(1, len(xs)):
                    w = xs[s_][1]
                    r0 = seg_off[s_] - seg_off[1]
                    wb.copy(WT[r0: r0 + w, :Pt], W[:, off: off + w].t())
                    off += w
                dXcat = torch.empty((N, sum(seg_pad)), dtype=act, device=dev)
                ops.linear_fwd(mode, _ksegs([(dZ, Pt)]), WT, ncols, out=dXcat[:, seg_off[1]:])

        # ---- DynEdgeConv layers, last first
        for l in reversed(range(nconv)):
            W1, b1, W2, b2 = conv_p[l]
            xin, Fin = xs[l]
            H1, H2 = int(W1.shape[0]), int(W2.shape[0])
            H1p = ops.round_up(H1, 32)
            g, PQ, mask = ctx.graphs[l], ctx.PQs[l], ctx.masks[l]
            g_out = dXcat[:, seg_off[l + 1]: seg_off[l + 1] + H2]
            dPQ = torch.empty((N, 2 * H1p), dtype=act, device=dev)
            dW2, db2 = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, g_out, mask)   # also records h>0 bits
            if ops.dpre_compact_supported(mode, g, H1p, H1, H2):
                # the edge-row tensor between the backward kernel and the source gather without its zero elements
                ops.edgeconv_bwd_gather_compact(g, PQ, H1p, H1, H2, g_out, mask, _packed(wb, ("W2T", l), W2.t(), dt), dPQ)
            else:
                dpre = torch.empty((max(g.rows, 1), H1p), dtype=dt, device=dev)
                ops.edgeconv_bwd(mode, g, PQ, H1p, H2, g_out, mask, _packed(wb, ("W2T", l), W2.t(), dt), dpre,
                                 dPQ[:, :H1p])
                ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
            dWpq, dbpq = ops.linear_wgrad(mode, dPQ, 2 * H1p, _ksegs([(xin, Fin)]), with_bias=True)
            dWpq = dWpq[:, :Fin]
            dWp, dWq = dWpq[:H1], dWpq[H1p:H1p + H1]
            grads[4 * l] = torch.cat([dWp, dWq - dWp], dim=1)
            grads[4 * l + 1] = dbpq[:H1]
            grads[4 * l + 2] = dW2
            grads[4 * l + 3] = db2
            if l > 0:
                Wa, Wb = W1[:, :Fin], W1[:, Fin:]
                # d_in += [dP | dQ] . [(Wa - Wb) | Wb]: one K = 2 H1p contraction (weights-stationary, csrc/gemm_v2.hip)
                # that accumulates into the skip-cat gradient of the producing layer - one pass over d_in, not two
                WpqT = wb.get(("WpqT", l), (ops.round_up(Fin, 128), ops.round_up(2 * H1p, ku)), dt, dev)
                wb.copy(WpqT[:Fin, :H1], Wa.t(), Wb.t())
                wb.copy(WpqT[:Fin, H1p:H1p + H1], Wb.t())
                d_in = dXcat[:, seg_off[l]: seg_off[l] + Fin]
                ops.linear_fwd(mode, [(dPQ, 2 * H1p)], WpqT, Fin, out=d_in, accum=True)
        wb.end("bwd", dev)
        return (None, None) + tuple(grads)


class _DynEdgeGenericFunction(torch.autograd.Function):
    """Same contract as :class:`_DynEdgeFunction` for ``activation_layer="gelu"`` and / or
    ``add_norm_layer=True`` (``dynedge.py:160-167,198-231``): the edge MLP runs unfused on edge-row tensors
    (``csrc/generic.hip``), every Linear on the MFMA GEMM kernels, storage fp32.

    ``params``: per conv layer ``W1, b1, [g1, be1], W2, b2, [g2, be2]``, per post layer ``W, b, [g, be]``
    (LayerNorm weight / bias present iff ``cfg["norm"]``).

    ``cfg["fused_edge"]`` (LeakyReLU edge MLPs without LayerNorm: ``DynEdgeJINST``): the convolution layers run on the
    fused edge kernels (``gn_edgeconv_leaky_fwd / _dw2 / _bwd``: no edge-row tensor in HBM on the way forward, one on
    the way back) and the activations between kernels are stored in the mode's activation type, as in
    :class:`_DynEdgeFunction`; the post-processing layers keep the row kernels of ``csrc/generic.hip``."""

    @staticmethod
    def _split(cfg, params):
        step = 4 if cfg["norm"] else 2
        conv, off = [], 0
        for _ in range(cfg["nconv"]):
            conv.append((params[off: off + step], params[off + step: off + 2 * step]))
            off += 2 * step
        post = [params[off + step * t: off + step * (t + 1)] for t in range(cfg["npost"])]
        return conv, post

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, *params: Tensor) -> Tensor:  # type: ignore[override]
        mode, act = cfg["mode"], cfg["act"]
        dt, ku = ops.mode_dtype(mode), ops.gemm_kunit(mode)
        batch, ptr, g = cfg["batch"], cfg["ptr"], cfg["graph"]
        conv_p, post_p = _DynEdgeGenericFunction._split(cfg, params)
        N, F = int(x.shape[0]), int(x.shape[1])
        gv = cfg["globals"]
        G = 0 if (gv is None or cfg["globals_after"]) else int(gv.shape[1])
        F0 = F + G
        fused = bool(cfg.get("fused_edge")) and act in ("relu", "leaky_relu") and not cfg["norm"]
        lowp = fused and mode == ops.MODE_BF16
        op_lowp = "only" if mode == ops.MODE_BF16 else "no"       # unfused layers: tensors that are GEMM operands and nothing else
        adt = ops.act_dtype(mode) if fused else torch.float32
        x0 = ops.concat_globals(x, gv if G else None, batch, ops.round_up(F0, 32), dtype=adt)
        xs: List[Tuple[Tensor, int]] = [(x0, F0)]
        graphs, saved, knn_coords = [], [], []
        plan = cfg.get("plan")
        nconv = cfg["nconv"]
        for l, (p1, p2) in enumerate(conv_p):
            W1, b1, W2, b2 = p1[0], p1[1], p2[0], p2[1]
            ln1 = (p1[2], p1[3]) if cfg["norm"] else (None, None)
            ln2 = (p2[2], p2[3]) if cfg["norm"] else (None, None)
            xin, Fin = xs[-1]
            H1, H2 = int(W1.shape[0]), int(W2.shape[0])
            H1p, H2r = ops.round_up(H1, 32), ops.round_up(H2, 8)
            Wa, Wb = W1[:, :Fin], W1[:, Fin:]
            Wpq = torch.zeros((2 * H1p, Fin), dtype=torch.float32, device=x.device)
            Wpq[:H1] = Wa - Wb
            Wpq[H1p:H1p + H1] = Wb
            bpq = torch.zeros(2 * H1p, dtype=torch.float32, device=x.device)
            bpq[:H1] = b1
            if fused:
                PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), ops.pack_weight(Wpq, [Fin], dt, ku), 2 * H1p, bias=bpq,
                                    out_lowp=lowp)
                W2p = ops.pack_weight(W2, [H1], dt, 32)
                cols = _subset_cols(cfg["features_subset"], H2) if l + 1 < nconv else None
                g_here = g
                if cols is not None and plan is None:
                    plan = ops.knn_plan(ptr, N)
                if cols is not None and lowp and len(cols) <= 8:
                    # bf16 activations: the k-NN coordinates leave the kernel as a separate fp32 copy
                    out, mask, coords = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2.contiguous(), H2, coord_cols=cols, H1=H1,
                                                         act=act)
                    g = ops.knn_graph(coords, list(range(len(cols))), batch, ptr, cfg["k"], strict=cfg["strict"], plan=plan)
                    knn_coords.append(coords[:, :len(cols)])
                else:
                    out, mask = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2.contiguous(), H2, H1=H1, act=act)
                    if cols is not None:
                        src = out.float() if lowp else out
                        g = ops.knn_graph(src, cols, batch, ptr, cfg["k"], strict=cfg["strict"], plan=plan)
                        knn_coords.append(src[:, cols])
                graphs.append(g_here)
                saved.append((PQ, mask))
                xs.append((out, H2))
                continue
            PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), ops.pack_weight(Wpq, [Fin], dt, ku), 2 * H1p, bias=bpq)
            # edge rows: the existing edges only (compact: N k + overflow rows; the slot layout has 16 slots for k = 9)
            cr = ops.compact_rows(g) if cfg.get("compact_rows", True) else None
            ic, jc = (cr.ic, cr.jc) if cr is not None else ops.edge_rows(g)
            # bf16 mode on compact rows: every edge-row tensor is stored in bf16 (the pre-activations the backward needs
            # included; LayerNorm statistics, sums and everything per pulse stay fp32)
            rows16 = op_lowp == "only" and cr is not None
            pre1 = ops.edge_gather_pre(PQ, H1p, ic, jc, lowp=rows16)
            # a1 is a GEMM operand only (forward and weight gradient): in bf16 mode it is stored in bf16 - the values the
            # GEMM kernels round their fp32 operand to anyway
            a1, st1 = ops.rownorm_act_fwd(pre1, H1, act, ln1[0], ln1[1], valid=jc, cpad=H1p, lowp=op_lowp)
            z2 = ops.linear_fwd(mode, [(a1, H1p)], ops.pack_weight(W2, [H1], dt, ku), H2, bias=b2.contiguous(),
                                out_cols=H2r, out_lowp=rows16)
            m, st2 = ops.rownorm_act_fwd(z2, H2, act, ln2[0], ln2[1], valid=jc, cpad=H2r, lowp="only" if rows16 else "no")
            out = cr.sum(m, H2) if cr is not None else ops.slot_sum(m, H2, g)
            graphs.append(g)
            # lean: keep only P|Q ([N, 2 H1p]) and rebuild the three edge-row tensors in the backward (same kernels, same
            # bits) - the [E, H] tensors of four layers are 23 GB at 1.6e5 pulses and do not fit at 6.2e5
            saved.append((PQ,) if cfg.get("lean") else (pre1, a1, st1, z2, st2))
            xs.append((out, H2))
            if l + 1 < nconv:
                cols = _subset_cols(cfg["features_subset"], H2)
                if plan is None:
                    plan = ops.knn_plan(ptr, N)
                g = ops.knn_graph(out, cols, batch, ptr, cfg["k"], strict=cfg["strict"], plan=plan)
                knn_coords.append(out[:, cols])
        zs, sts = [], []
        segs = xs
        post_acts = cfg.get("post_acts") or [act] * cfg["npost"]
        for t, (pp) in enumerate(post_p):
            W, b = pp[0], pp[1]
            gam, bet = (pp[2], pp[3]) if cfg["norm"] else (None, None)
            P_ = int(W.shape[0])
            z = ops.linear_fwd(mode, _ksegs(segs), ops.pack_weight(W, [w for _, w in segs], dt, ku), P_,
                               bias=b.contiguous(), out_cols=ops.round_up(P_, 8))
            # (fused convolutions in bf16 mode: a hidden post-processing layer's output is only a GEMM operand -> bf16)
            y, st = ops.rownorm_act_fwd(z, P_, post_acts[t], gam, bet, cpad=ops.round_up(P_, 8),
                                        lowp="only" if lowp and t + 1 < cfg["npost"] else "no")
            zs.append(z); sts.append(st)
            segs = [(y, P_)]
        y_last, P = segs[0]
        ctx.cfg, ctx.xs, ctx.graphs, ctx.saved, ctx.zs, ctx.sts, ctx.params = cfg, xs, graphs, saved, zs, sts, params
        ctx.amin = ctx.amax = None
        ctx.fused = fused
        cfg["trace"] = ({"conv_out": [t.float() for t, _ in xs], "graphs": graphs, "post": y_last[:, :P],
                         "knn_coords": knn_coords} if cfg.get("want_trace") else None)
        if cfg["pools"]:
            pooled, ctx.amin, ctx.amax = ops.segment_pool_fwd(y_last, P, ptr, cfg["pools"])
            return pooled
        return y_last[:, :P] if int(y_last.shape[1]) != P else y_last

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        cfg = ctx.cfg
        mode, act = cfg["mode"], cfg["act"]
        dt, ku = ops.mode_dtype(mode), ops.gemm_kunit(mode)
        batch, ptr = cfg["batch"], cfg["ptr"]
        params = ctx.params
        conv_p, post_p = _DynEdgeGenericFunction._split(cfg, params)
        step = 4 if cfg["norm"] else 2
        nconv, npost = cfg["nconv"], cfg["npost"]
        xs = ctx.xs
        N, dev = int(xs[0][0].shape[0]), xs[0][0].device
        grads: List[Optional[Tensor]] = [None] * len(params)
        post_base = 2 * step * nconv
        P = int(post_p[-1][0].shape[0])
        gout = gout.contiguous().to(torch.float32)
        if cfg["pools"]:
            gy = ops.segment_pool_bwd(gout, P, ptr, batch, N, cfg["pools"], ctx.amin, ctx.amax, None)
        else:
            gy = torch.zeros((N, ops.round_up(P, 8)), dtype=torch.float32, device=dev)
            gy[:, :P] = gout

        post_acts = cfg.get("post_acts") or [act] * npost
        seg_pad = [ops.round_up(w, 32) for _, w in xs]
        seg_off = [sum(seg_pad[:i]) for i in range(len(xs))]
        dXcat = None
        fused = ctx.fused
        adt = ops.act_dtype(mode) if fused else torch.float32
        op_lowp = "only" if mode == ops.MODE_BF16 else "no"
        for t in reversed(range(npost)):
            pp = post_p[t]
            W = pp[0]
            gam, bet = (pp[2], pp[3]) if cfg["norm"] else (None, None)
            Pt = int(W.shape[0])
            lowp = adt == torch.bfloat16              # fused convolutions, bf16 mode: the GEMM operands dz / yprev in bf16
            dz, dgam, dbet = ops.rownorm_act_bwd(gy, ctx.zs[t], Pt, post_acts[t], gam, bet, ctx.sts[t],
                                                 cpad=ops.round_up(Pt, 8), lowp="only" if lowp else "no")
            in_segs = xs if t == 0 else [(None, int(post_p[t - 1][0].shape[0]))]
            if t > 0:   # input of layer t = activation output of layer t-1: recompute it from the saved z
                pq = post_p[t - 1]
                gq, bq = (pq[2], pq[3]) if cfg["norm"] else (None, None)
                Pprev = int(pq[0].shape[0])
                yprev, _ = ops.rownorm_act_fwd(ctx.zs[t - 1], Pprev, post_acts[t - 1], gq, bq, cpad=ops.round_up(Pprev, 8),
                                               lowp="only" if lowp else "no")
                in_segs = [(yprev, Pprev)]
            dWt, dbt = ops.linear_wgrad(mode, dz, Pt, _ksegs(in_segs), with_bias=True)
            base = post_base + step * t
            grads[base] = _unpad_cols(dWt, [w for _, w in in_segs], ops.seg_unit(in_segs[0][0].dtype))
            grads[base + 1] = dbt
            if cfg["norm"]:
                grads[base + 2], grads[base + 3] = dgam, dbet
            if t > 0:
                gy = ops.linear_fwd(mode, _ksegs([(dz, Pt)]), ops.pack_weight(W.t(), [Pt], dt, ku), Pprev,
                                    out_cols=ops.round_up(Pprev, 8))
            else:
                WT = torch.zeros((sum(seg_pad), Pt), dtype=torch.float32, device=dev)
                off = 0
                for s_, (_, w) in enumerate(xs):
                    WT[seg_off[s_]: seg_off[s_] + w] = W[:, off: off + w].t()
                    off += w
                dXcat = ops.linear_fwd(mode, _ksegs([(dz, Pt)]), ops.pack_weight(WT, [Pt], dt, ku), sum(seg_pad),
                                       out_lowp=adt == torch.bfloat16)

        for l in reversed(range(nconv)):
            p1, p2 = conv_p[l]
            W1, W2 = p1[0], p2[0]
            ln1 = (p1[2], p1[3]) if cfg["norm"] else (None, None)
            ln2 = (p2[2], p2[3]) if cfg["norm"] else (None, None)
            xin, Fin = xs[l]
            H1, H2 = int(W1.shape[0]), int(W2.shape[0])
            H1p, H2r = ops.round_up(H1, 32), ops.round_up(H2, 8)
            g = ctx.graphs[l]
            g_out = dXcat[:, seg_off[l + 1]: seg_off[l + 1] + H2]
            dg1 = db1n = dg2 = db2n = None
            if fused:
                PQ, mask = ctx.saved[l]
                dPQ = torch.empty((N, 2 * H1p), dtype=adt, device=dev)
                dW2, db2 = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, g_out, mask, act=act)     # also records the h > 0 bits
                dpre = torch.empty((max(g.rows, 1), H1p), dtype=dt, device=dev)
                ops.edgeconv_bwd(mode, g, PQ, H1p, H2, g_out, mask, ops.pack_weight(W2.t().contiguous(), [H2], dt, 32), dpre,
                                 dPQ[:, :H1p], act=act, H1=H1)
                ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
            else:
                cr = ops.compact_rows(g) if cfg.get("compact_rows", True) else None
                ic, jc = (cr.ic, cr.jc) if cr is not None else ops.edge_rows(g)
                rows16 = op_lowp == "only" and cr is not None
                if len(ctx.saved[l]) == 1:               # lean: rebuild the forward's edge-row tensors of this layer
                    (PQ,) = ctx.saved[l]
                    pre1 = ops.edge_gather_pre(PQ, H1p, ic, jc, lowp=rows16)
                    a1, st1 = ops.rownorm_act_fwd(pre1, H1, act, ln1[0], ln1[1], valid=jc, cpad=H1p, lowp=op_lowp)
                    z2 = ops.linear_fwd(mode, [(a1, H1p)], ops.pack_weight(W2, [H1], dt, ku), H2, bias=p2[1].contiguous(),
                                        out_cols=H2r, out_lowp=rows16)
                    _, st2 = ops.rownorm_act_fwd(z2, H2, act, ln2[0], ln2[1], valid=jc, cpad=H2r)
                    del PQ, _
                else:
                    pre1, a1, st1, z2, st2 = ctx.saved[l]
                # dz2: operand of the two GEMMs below and nothing else (bf16 mode: stored in bf16; db2 is then summed from the rounded values)
                dz2, dg2, db2n = ops.rownorm_act_bwd(g_out, z2, H2, act, ln2[0], ln2[1], st2, valid=jc, gidx=ic, cpad=H2r,
                                                     lowp=op_lowp)
                dW2, db2 = ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
                da1 = ops.linear_fwd(mode, _ksegs([(dz2, H2)]), ops.pack_weight(W2.t(), [H2], dt, ku), H1, out_cols=H1p,
                                     out_lowp=rows16)
                dpre1, dg1, db1n = ops.rownorm_act_bwd(da1, pre1, H1, act, ln1[0], ln1[1], st1, valid=jc, cpad=H1p,
                                                       lowp="only" if rows16 else "no")
                dPQ = torch.empty((N, 2 * H1p), dtype=torch.bfloat16 if rows16 else torch.float32, device=dev)
                if cr is not None:
                    dPQ[:, :H1p] = cr.sum(dpre1, H1p)
                    ops.edgeconv_dq_gather(ops.MODE_BF16 if rows16 else ops.MODE_F32, cr.reverse_view(), dpre1, H1p, dPQ[:, H1p:])
                else:
                    dPQ[:, :H1p] = ops.slot_sum(dpre1, H1p, g)
                    ops.edgeconv_dq_gather(ops.MODE_F32, g, dpre1, H1p, dPQ[:, H1p:])
                del pre1, a1, z2, dz2, da1, dpre1
            dWpq, dbpq = ops.linear_wgrad(mode, dPQ, 2 * H1p, _ksegs([(xin, Fin)]), with_bias=True)
            dWpq = dWpq[:, :Fin]
            dWp, dWq = dWpq[:H1], dWpq[H1p:H1p + H1]
            base = 2 * step * l
            grads[base] = torch.cat([dWp, dWq - dWp], dim=1)
            grads[base + 1] = dbpq[:H1]
            grads[base + step] = dW2[:, :H1]
            grads[base + step + 1] = db2
            if cfg["norm"]:
                grads[base + 2], grads[base + 3] = dg1, db1n
                grads[base + step + 2], grads[base + step + 3] = dg2, db2n
            if l > 0:
                Wa, Wb = W1[:, :Fin], W1[:, Fin:]
                WpqT = torch.zeros((Fin, 2 * H1p), dtype=torch.float32, device=dev)
                WpqT[:, :H1] = (Wa - Wb).t()
                WpqT[:, H1p:H1p + H1] = Wb.t()
                ops.linear_fwd(mode, [(dPQ, 2 * H1p)], ops.pack_weight(WpqT, [2 * H1p], dt, ku), Fin,
                               out=dXcat[:, seg_off[l]: seg_off[l] + Fin], accum=True)
        return (None, None) + tuple(grads)


class DynEdge(GNN):
    """DynEdge (dynamical edge convolutional) model on hand-written gfx950 kernels.

    Constructor arguments are those of the reference (``dynedge.py:24-38``).  Extra,
    keyword-only backend switches (not part of the reference config) are set afterwards with
    :meth:`set_backend`.
    """

    def __init__(
        self,
        nb_inputs: int,
        *,
        nb_neighbours: int = 8,
        features_subset: Optional[Union[List[int], slice]] = None,
        dynedge_layer_sizes: Optional[List[Tuple[int, ...]]] = None,
        post_processing_layer_sizes: Optional[List[int]] = None,
        readout_layer_sizes: Optional[List[int]] = None,
        global_pooling_schemes: Optional[Union[str, List[str]]] = None,
        add_global_variables_after_pooling: bool = False,
        activation_layer: Optional[str] = None,
        add_norm_layer: bool = False,
        skip_readout: bool = False,
    ):
        if features_subset is None:
            features_subset = slice(0, 3)
        if dynedge_layer_sizes is None:
            dynedge_layer_sizes = [(128, 256), (336, 256), (336, 256), (336, 256)]
        assert isinstance(dynedge_layer_sizes, list)
        assert len(dynedge_layer_sizes)
        assert all(isinstance(sizes, tuple) for sizes in dynedge_layer_sizes)
        assert all(len(sizes) > 0 for sizes in dynedge_layer_sizes)
        assert all(all(size > 0 for size in sizes) for sizes in dynedge_layer_sizes)
        self._dynedge_layer_sizes = dynedge_layer_sizes

        if post_processing_layer_sizes is None:
            post_processing_layer_sizes = [336, 256]
        assert isinstance(post_processing_layer_sizes, list)
        assert len(post_processing_layer_sizes)
        assert all(size > 0 for size in post_processing_layer_sizes)
        self._post_processing_layer_sizes = post_processing_layer_sizes

        if readout_layer_sizes is None:
            readout_layer_sizes = [128]
        assert isinstance(readout_layer_sizes, list)
        assert len(readout_layer_sizes)
        assert all(size > 0 for size in readout_layer_sizes)
        self._readout_layer_sizes = readout_layer_sizes

        if isinstance(global_pooling_schemes, str):
            global_pooling_schemes = [global_pooling_schemes]
        if isinstance(global_pooling_schemes, list):
            for pooling_scheme in global_pooling_schemes:
                assert pooling_scheme in GLOBAL_POOLINGS, f"Global pooling scheme {pooling_scheme} not supported."
        else:
            assert global_pooling_schemes is None
        self._global_pooling_schemes = global_pooling_schemes

        if add_global_variables_after_pooling:
            assert self._global_pooling_schemes, (
                "No global pooling schemes were request, so cannot add global variables after pooling."
            )
        self._add_global_variables_after_pooling = add_global_variables_after_pooling

        if activation_layer is None or activation_layer.lower() == "relu":
            activation: torch.nn.Module = torch.nn.ReLU()
        elif activation_layer.lower() == "gelu":
            activation = torch.nn.GELU()
        else:
            raise ValueError(f"Activation layer {activation_layer} not supported.")

        super().__init__(nb_inputs, self._readout_layer_sizes[-1])

        self._activation = activation
        self._nb_inputs = nb_inputs
        self._nb_global_variables = 5 + nb_inputs
        self._nb_neighbours = nb_neighbours
        self._features_subset = features_subset
        self._add_norm_layer = add_norm_layer
        self._skip_readout = skip_readout
        # backend switches (see set_backend)
        self._compute_mode = ops.MODE_BF16
        self._knn_strict = False
        self._graph_columns = [0, 1, 2]
        self._construct_layers()

    # reference: dynedge.py:183-249 (same module tree, same parameter names)
    def _construct_layers(self) -> None:
        nb_input_features = self._nb_inputs
        if not self._add_global_variables_after_pooling:
            nb_input_features += self._nb_global_variables
        self._conv_layers = torch.nn.ModuleList()
        nb_latent_features = nb_input_features
        nb_out = nb_latent_features
        for sizes in self._dynedge_layer_sizes:
            layers: List[torch.nn.Module] = []
            layer_sizes = [nb_latent_features] + list(sizes)
            for ix, (nb_in, nb_out) in enumerate(zip(layer_sizes[:-1], layer_sizes[1:])):
                if ix == 0:
                    nb_in *= 2
                layers.append(torch.nn.Linear(nb_in, nb_out))
                if self._add_norm_layer:
                    layers.append(torch.nn.LayerNorm(nb_out))
                layers.append(self._activation)
            self._conv_layers.append(
                _ConvParams(torch.nn.Sequential(*layers), self._nb_neighbours, self._features_subset))
            nb_latent_features = nb_out

        nb_latent_features = sum(sizes[-1] for sizes in self._dynedge_layer_sizes) + nb_input_features
        post_processing_layers: List[torch.nn.Module] = []
        layer_sizes = [nb_latent_features] + list(self._post_processing_layer_sizes)
        for nb_in, nb_out in zip(layer_sizes[:-1], layer_sizes[1:]):
            post_processing_layers.append(torch.nn.Linear(nb_in, nb_out))
            if self._add_norm_layer:
                post_processing_layers.append(torch.nn.LayerNorm(nb_out))
            post_processing_layers.append(self._activation)
        self._post_processing = torch.nn.Sequential(*post_processing_layers)

        nb_poolings = len(self._global_pooling_schemes) if self._global_pooling_schemes else 1
        nb_latent_features = nb_out * nb_poolings
        if self._add_global_variables_after_pooling:
            nb_latent_features += self._nb_global_variables
        readout_layers: List[torch.nn.Module] = []
        layer_sizes = [nb_latent_features] + list(self._readout_layer_sizes)
        for nb_in, nb_out in zip(layer_sizes[:-1], layer_sizes[1:]):
            readout_layers.append(torch.nn.Linear(nb_in, nb_out))
            readout_layers.append(self._activation)
        self._readout = torch.nn.Sequential(*readout_layers)

    # ------------------------------------------------------------------ backend control
    def set_backend(self, *, dtype: str = "bf16", knn_mode: str = "compat",
                    graph_columns: Optional[List[int]] = None, overlap: Optional[bool] = None,
                    step_entry: Optional[bool] = None) -> "DynEdge":
        """``dtype``: "bf16" (MFMA bf16 operands, fp32 accumulate) or "fp32" (exact-f32 MFMA,
        parity mode).  ``knn_mode``: "compat" (k+1-with-self then mask, as knn_graph) or
        "strict".  ``graph_columns``: columns for the layer-1 k-NN when the batch carries no
        ``edge_index`` (KNNGraph default ``[0, 1, 2]``, ``graphs/graphs.py:25``)."""
        self._compute_mode = {"bf16": ops.MODE_BF16, "fp32": ops.MODE_F32, "f32": ops.MODE_F32}[dtype]
        self._knn_strict = {"compat": False, "strict": True}[knn_mode]
        if graph_columns is not None:
            self._graph_columns = list(graph_columns)
        if overlap is not None:     # graph building on a second HIP stream beside the GEMM / edge kernels (default off)
            self._overlap = bool(overlap)
        if step_entry is not None:  # the whole pass behind one C entry (default on; False: one ctypes call per op)
            self._step_entry = bool(step_entry)
        return self

    def _stepper(self, F: int):
        """The one-call path (``gn_dynedge_fwd`` / ``gn_dynedge_bwd``, csrc/step.hip) for this configuration, or None:
        relu edge MLPs of two layers, pooled output, no second stream.  ``GN_STEP_ENTRY=0`` switches it off."""
        from .step import DynEdgeStepper
        if self._is_generic() or self._skip_readout or not self._global_pooling_schemes or \
                not getattr(self, "_step_entry", True) or os.environ.get("GN_STEP_ENTRY", "1") == "0":
            return None
        conv = [tuple(s) for s in self._dynedge_layer_sizes]
        post = list(self._post_processing_layer_sizes)
        knn_cols = _subset_cols(self._features_subset, conv[0][-1]) if all(len(s) == 2 for s in conv) else []
        if not DynEdgeStepper.supported(len(conv), len(post), conv, self._global_pooling_schemes, len(knn_cols)):
            return None
        G = 0 if self._add_global_variables_after_pooling else F + 5
        key = (self._compute_mode, F, G, self._nb_neighbours, self._knn_strict, tuple(self._graph_columns), tuple(knn_cols))
        cache = self.__dict__.setdefault("_steppers", {})
        st = cache.get(key)
        if st is None:
            st = DynEdgeStepper(self._compute_mode, F, G, self._nb_neighbours, self._knn_strict, self._graph_columns, knn_cols,
                                conv, post, self._global_pooling_schemes)
            cache[key] = st
        return st

    def _side_stream(self, device, n_pulses: int) -> Optional["torch.cuda.Stream"]:
        """Second HIP stream for graph building: opt-in (``set_backend(overlap=True)``), never during hipGraph
        capture.  Off by default: the persistent edge kernels occupy every CU for their whole run, and whether the
        side stream's small kernels (scans of the reverse-adjacency build) get wave slots beside them is up to the
        hardware dispatcher - measured from +1 % (26.3 -> 26.0 ms at B = 4096) to -40 % (36.8 ms: every scan
        launch waited ~0.86 ms behind an edge kernel and the join stalled the main stream)."""
        if not getattr(self, "_overlap", False) or os.environ.get("GN_NO_OVERLAP") == "1" or \
                torch.cuda.is_current_stream_capturing():
            return None
        st = self.__dict__.get("_side")
        if st is None:
            st = torch.cuda.Stream(device=device)
            self.__dict__["_side"] = st
        return st

    def _is_generic(self) -> bool:
        """GELU and / or LayerNorm: the unfused kernels of csrc/generic.hip (the fused path is relu, no norm)."""
        return not isinstance(self._activation, torch.nn.ReLU) or self._add_norm_layer

    def _check_supported(self) -> None:
        if not isinstance(self._activation, (torch.nn.ReLU, torch.nn.GELU)):
            raise NotImplementedError("graphnet_amd.DynEdge: activation must be relu or gelu (no fallback)")
        if any(len(s) != 2 for s in self._dynedge_layer_sizes):
            raise NotImplementedError("graphnet_amd.DynEdge: each DynEdgeConv MLP must have exactly two layers.")

    def _csr(self, data: Any, x: Tensor):
        N = int(x.shape[0])
        n_pulses = data.n_pulses.to(torch.int32)
        ptr = _maybe(data, "ptr")
        if ptr is None:
            ptr = torch.zeros(n_pulses.shape[0] + 1, dtype=torch.int64, device=x.device)
            ptr[1:] = torch.cumsum(torch.bincount(data.batch, minlength=n_pulses.shape[0]), 0)
        ptr32 = ptr.to(torch.int32)
        batch = _maybe(data, "batch")
        batch32 = batch.to(torch.int32) if batch is not None else ops.ptr_to_batch(ptr32, N)
        return ptr32, batch32, n_pulses

    def _layer0_graph(self, data: Any, x: Tensor, batch32: Tensor, ptr32: Tensor) -> ops.NeighbourTable:
        table = _maybe(data, "nbr_table")
        if isinstance(table, ops.NeighbourTable):
            return table
        ei = _maybe(data, "edge_index")
        if ei is not None:
            return ops.table_from_edge_index(ei, int(x.shape[0]), self._nb_neighbours)
        mink = minkowski_record(data)
        if mink is not None:        # recorded by MinkowskiKNNEdges on a CPU Data: one launch for the whole batch, here
            k, c, tlw, time_coord, space_coords = mink
            plan = ops.knn_plan(ptr32, int(x.shape[0]))
            self.__dict__["_last_plan"] = plan
            return ops.minkowski_knn_graph(x, space_coords, time_coord, c, tlw, batch32, ptr32, k, plan=plan)
        radial = radial_record(data)
        if radial is not None:      # recorded by RadialEdges on a CPU Data: one launch for the whole batch, here
            r, rcols, cap = radial
            plan = ops.knn_plan(ptr32, int(x.shape[0]))
            self.__dict__["_last_plan"] = plan
            return ops.radius_graph(x, rcols, r, batch32, ptr32, cap, plan=plan)
        k, cols = self._nb_neighbours, self._graph_columns
        knn_k = _maybe(data, "knn_k")
        if knn_k is not None:       # recorded by KNNEdges on a CPU Data: same k / columns, built here
            k = int(knn_k.reshape(-1)[0]) if isinstance(knn_k, Tensor) else int(knn_k)
            kc = _maybe(data, "knn_columns")
            cols = list(kc[0]) if isinstance(kc, list) and kc and isinstance(kc[0], (list, tuple)) else list(kc)
        plan = ops.knn_plan(ptr32, int(x.shape[0]))
        self.__dict__["_last_plan"] = plan
        return ops.knn_graph(x, cols, batch32, ptr32, k, strict=self._knn_strict, plan=plan, sweep=True)

    def _weight_buffers(self) -> _WeightBuffers:
        wb = self.__dict__.get("_wbuf")
        if wb is None:
            wb = _WeightBuffers()
            self.__dict__["_wbuf"] = wb          # plain attribute: not a module / parameter / buffer
        return wb

    def _generic_params(self) -> List[Tensor]:
        """Linear (and LayerNorm) parameters in module order: conv MLPs, then the post-processing MLP."""
        ps: List[Tensor] = []
        for seq in [conv.nn for conv in self._conv_layers] + [self._post_processing]:
            for m in seq:
                if isinstance(m, (torch.nn.Linear, torch.nn.LayerNorm)):
                    ps += [m.weight, m.bias]
        return ps

    def _kernel_params(self) -> List[Tensor]:
        ps: List[Tensor] = []
        for conv in self._conv_layers:
            lin = [m for m in conv.nn if isinstance(m, torch.nn.Linear)]
            ps += [lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias]
        for m in self._post_processing:
            if isinstance(m, torch.nn.Linear):
                ps += [m.weight, m.bias]
        return ps

    def forward(self, data: Any, return_trace: bool = False) -> Tensor:
        """Apply learnable forward pass (``dynedge.py:295-349``)."""
        self._check_supported()
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.DynEdge runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        x = x.to(torch.float32)
        ptr32, batch32, n_pulses = self._csr(data, x)
        stepper = None if return_trace or self._side_stream(x.device, int(x.shape[0])) is not None or \
            int(x.shape[0]) < 1 or int(ptr32.shape[0]) < 2 else self._stepper(int(x.shape[1]))
        if stepper is not None:
            from .step import DynEdgeStepFunction
            box: dict = {}
            if isinstance(_maybe(data, "nbr_table"), ops.NeighbourTable) or _maybe(data, "edge_index") is not None or \
                    _maybe(data, "knn_k") is not None or _maybe(data, "mink_k") is not None or \
                    _maybe(data, "radial_r") is not None:
                box["table"] = self._layer0_graph(data, x, batch32, ptr32)      # the caller's graph (or its k / columns)
            out = DynEdgeStepFunction.apply(stepper, box, x.contiguous(), ptr32, batch32, n_pulses, *self._kernel_params())
            if self._add_global_variables_after_pooling:
                out = torch.cat([out, box["global_variables"]], dim=1)
            return self._readout(out)
        self.__dict__["_last_plan"] = None
        g0 = self._layer0_graph(data, x, batch32, ptr32)
        gv = ops.graph_globals(x, ptr32, g0, n_pulses)
        cfg = {
            "mode": self._compute_mode, "batch": batch32, "ptr": ptr32, "graph": g0,
            "nconv": len(self._conv_layers),
            "npost": sum(isinstance(m, torch.nn.Linear) for m in self._post_processing),
            "globals": gv, "globals_after": self._add_global_variables_after_pooling,
            "features_subset": self._features_subset, "k": self._nb_neighbours, "strict": self._knn_strict,
            "pools": None if self._skip_readout else self._global_pooling_schemes,
            "want_trace": return_trace, "wbuf": self._weight_buffers(), "plan": self.__dict__.get("_last_plan"), "side_stream": self._side_stream(x.device, int(x.shape[0])),
        }
        if self._is_generic():
            cfg["act"] = "gelu" if isinstance(self._activation, torch.nn.GELU) else "relu"
            cfg["norm"] = bool(self._add_norm_layer)
            # edge-row tensors the backward needs, all layers, fp32: above a quarter of the device's memory they are rebuilt
            # in the backward instead of kept (GN_GENERIC_LEAN=0 / 1 forces either)
            cfg["compact_rows"] = os.environ.get("GN_GENERIC_COMPACT", "1") != "0"
            rows = int(x.shape[0]) * ((self._nb_neighbours if cfg["compact_rows"] else
                                       int(ops._lib.lib().gn_edge_slots(self._nb_neighbours))) + 1)
            esz = 2 if (cfg["compact_rows"] and self._compute_mode == ops.MODE_BF16) else 4
            keep = sum(esz * rows * (2 * ops.round_up(a, 32) + ops.round_up(b_, 8)) for a, b_ in self._dynedge_layer_sizes)
            env = os.environ.get("GN_GENERIC_LEAN")
            cfg["lean"] = (env == "1") if env in ("0", "1") else \
                keep > 0.25 * torch.cuda.get_device_properties(x.device).total_memory
            out = _DynEdgeGenericFunction.apply(cfg, x, *self._generic_params())
        else:
            out = _DynEdgeFunction.apply(cfg, x, *self._kernel_params())
        if not self._skip_readout:
            if self._global_pooling_schemes and self._add_global_variables_after_pooling:
                out = torch.cat([out, gv], dim=1)
            out = self._readout(out)
        if return_trace:
            trace = cfg["trace"] or {}
            trace["global_variables"] = gv
            return out, trace
        return out


class DynEdgeJINST(GNN):
    """``DynEdgeJINST`` (``models/gnn/dynedge_jinst.py:16-161``, the architecture of arXiv:2209.03042) on the same
    kernels: four DynEdgeConv layers with LeakyReLU edge MLPs (the fused edge kernels in their leaky-relu variant:
    ``gn_edgeconv_leaky_*``), skip-cat, nn1 + LeakyReLU, nn2, max / min / sum / mean pooling, homophily and pulse
    count appended, LeakyReLU, nn3, LeakyReLU.  Same attribute names as the reference => same state-dict keys."""

    def __init__(self, nb_inputs: int, layer_size_scale: int = 4):
        c = layer_size_scale
        l1, l2, l3, l4, l5, l6 = nb_inputs, c * 16 * 2, c * 32 * 2, c * 42 * 2, c * 32 * 2, c * 16 * 2
        super().__init__(nb_inputs, l6)

        def mlp(a: int, b: int, cc: int) -> torch.nn.Sequential:
            return torch.nn.Sequential(torch.nn.Linear(a * 2, b), torch.nn.LeakyReLU(), torch.nn.Linear(b, cc),
                                       torch.nn.LeakyReLU())
        self.conv_add1 = _ConvParams(mlp(l1, l2, l3), 8, slice(0, 3))
        self.conv_add2 = _ConvParams(mlp(l3, l4, l3), 8, slice(0, 3))
        self.conv_add3 = _ConvParams(mlp(l3, l4, l3), 8, slice(0, 3))
        self.conv_add4 = _ConvParams(mlp(l3, l4, l3), 8, slice(0, 3))
        self.nn1 = torch.nn.Linear(l3 * 4 + l1, l4)
        self.nn2 = torch.nn.Linear(l4, l5)
        self.nn3 = torch.nn.Linear(4 * l5 + 5, l6)
        self.lrelu = torch.nn.LeakyReLU()
        self._compute_mode = ops.MODE_BF16
        self._knn_strict = False
        self._fused_edge = True

    def set_backend(self, dtype: Optional[str] = None, knn_mode: Optional[str] = None,
                    fused_edge: Optional[bool] = None) -> "DynEdgeJINST":
        """``fused_edge`` (default on): the convolution layers on the fused leaky-relu edge kernels
        (``gn_edgeconv_leaky_*``); off: the unfused edge-row kernels of ``csrc/generic.hip`` (A/B, parity tests)."""
        if dtype is not None:
            self._compute_mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
        if knn_mode is not None:
            self._knn_strict = {"compat": False, "strict": True}[knn_mode]
        if fused_edge is not None:
            self._fused_edge = bool(fused_edge)
        return self

    def forward(self, data: Any, return_trace: bool = False) -> Tensor:
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.DynEdgeJINST runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        x = x.to(torch.float32)
        ptr32, batch32, n_pulses = DynEdge._csr(self, data, x)
        ei = _maybe(data, "edge_index")
        _no_radial_record(data, ei, type(self).__name__)
        g0 = (ops.table_from_edge_index(ei, int(x.shape[0]), 8) if ei is not None
              else ops.knn_graph(x, [0, 1, 2], batch32, ptr32, 8, strict=self._knn_strict, sweep=True))
        gv = ops.graph_globals(x, ptr32, g0, n_pulses)          # [mean_F | h_x h_y h_z h_t | log10 n]
        F = int(x.shape[1])
        cfg = {
            "mode": self._compute_mode, "batch": batch32, "ptr": ptr32, "graph": g0, "nconv": 4, "npost": 2,
            "globals": None, "globals_after": True, "features_subset": slice(0, 3), "k": 8,
            "strict": self._knn_strict, "pools": ["max", "min", "sum", "mean"], "want_trace": return_trace,
            "act": "leaky_relu", "post_acts": ["leaky_relu", "identity"], "norm": False, "fused_edge": self._fused_edge,
        }
        params: List[Tensor] = []
        for conv in (self.conv_add1, self.conv_add2, self.conv_add3, self.conv_add4):
            params += [conv.nn[0].weight, conv.nn[0].bias, conv.nn[2].weight, conv.nn[2].bias]
        params += [self.nn1.weight, self.nn1.bias, self.nn2.weight, self.nn2.bias]
        pooled = _DynEdgeGenericFunction.apply(cfg, x, *params)
        h = gv[:, F: F + 4]
        feats = torch.cat([pooled, h[:, 3:4], h[:, 0:1], h[:, 1:2], h[:, 2:3],
                           n_pulses.reshape(-1, 1).to(pooled.dtype)], dim=1)
        out = self.lrelu(self.nn3(self.lrelu(feats)))
        if return_trace:
            trace = cfg["trace"] or {}
            trace["global_variables"] = gv
            return out, trace
        return out


# ------------------------------------------------------------------------------ stand-alone DynEdgeConv layer
_ACT_NAMES = {torch.nn.ReLU: "relu", torch.nn.GELU: "gelu", torch.nn.LeakyReLU: "leaky_relu", torch.nn.Identity: "identity"}


class _EdgeConvFunction(torch.autograd.Function):
    """One EdgeConv (``x_i' = aggr_j nn([x_i || x_j - x_i])``, two-layer ``nn``) on the unfused kernels;
    differentiable w.r.t. ``x`` and every parameter.  ``params``: W1, b1, [g1, be1], W2, b2, [g2, be2]."""

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, *params: Tensor) -> Tensor:  # type: ignore[override]
        mode, g, aggr, norm = cfg["mode"], cfg["graph"], cfg["aggr"], cfg["norm"]
        act1, act2 = cfg["acts"]
        dt, ku = ops.mode_dtype(mode), ops.gemm_kunit(mode)
        step = 4 if norm else 2
        p1, p2 = params[:step], params[step:]
        W1, b1, W2, b2 = p1[0], p1[1], p2[0], p2[1]
        ln1 = (p1[2], p1[3]) if norm else (None, None)
        ln2 = (p2[2], p2[3]) if norm else (None, None)
        N, Fin = int(x.shape[0]), int(x.shape[1])
        xin = torch.zeros((N, ops.round_up(Fin, 32)), dtype=torch.float32, device=x.device)
        xin[:, :Fin] = x
        H1, H2 = int(W1.shape[0]), int(W2.shape[0])
        H1p, H2r = ops.round_up(H1, 32), ops.round_up(H2, 8)
        Wa, Wb = W1[:, :Fin], W1[:, Fin:]
        Wpq = torch.zeros((2 * H1p, Fin), dtype=torch.float32, device=x.device)
        Wpq[:H1] = Wa - Wb
        Wpq[H1p:H1p + H1] = Wb
        bpq = torch.zeros(2 * H1p, dtype=torch.float32, device=x.device)
        bpq[:H1] = b1
        # add aggregation with ReLU or LeakyReLU after both layers, no LayerNorm: the fused edge kernels (gn_edgeconv_fwd /
        # gn_edgeconv_leaky_fwd) - no edge-row tensor in HBM; activations in the mode's type, result returned in fp32
        lowp = mode == ops.MODE_BF16
        ctx.fused = bool(cfg.get("fused", True)) and aggr == "add" and not norm and act1 == act2 and \
            act1 in ("relu", "leaky_relu") and (not lowp or H2 % 8 == 0)
        if ctx.fused:
            adt = ops.act_dtype(mode)
            xa = xin.to(adt)
            PQ = ops.linear_fwd(mode, _ksegs([(xa, Fin)]), ops.pack_weight(Wpq, [Fin], dt, ku), 2 * H1p, bias=bpq, out_lowp=lowp)
            out, mask = ops.edgeconv_fwd(mode, g, PQ, H1p, ops.pack_weight(W2, [H1], dt, 32), b2.contiguous(), H2, H1=H1, act=act1)
            ctx.cfg, ctx.params, ctx.saved = cfg, params, (xa, Fin, PQ, mask)
            return out.float() if lowp else out
        PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), ops.pack_weight(Wpq, [Fin], dt, ku), 2 * H1p, bias=bpq)
        ic, jc = ops.edge_rows(g)
        pre1 = ops.edge_gather_pre(PQ, H1p, ic, jc)
        a1, st1 = ops.rownorm_act_fwd(pre1, H1, act1, ln1[0], ln1[1], valid=jc, cpad=H1p)
        z2 = ops.linear_fwd(mode, [(a1, H1p)], ops.pack_weight(W2, [H1], dt, ku), H2, bias=b2.contiguous(), out_cols=H2r)
        m, st2 = ops.rownorm_act_fwd(z2, H2, act2, ln2[0], ln2[1], valid=jc, cpad=H2r)
        out, aux = ops.slot_reduce(m, H2, g, aggr)
        ctx.cfg, ctx.params, ctx.saved = cfg, params, (xin, Fin, pre1, a1, st1, z2, st2, aux)
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        cfg, params = ctx.cfg, ctx.params
        mode, g, aggr, norm = cfg["mode"], cfg["graph"], cfg["aggr"], cfg["norm"]
        act1, act2 = cfg["acts"]
        dt, ku = ops.mode_dtype(mode), ops.gemm_kunit(mode)
        step = 4 if norm else 2
        p1, p2 = params[:step], params[step:]
        W1, W2 = p1[0], p2[0]
        ln1 = (p1[2], p1[3]) if norm else (None, None)
        ln2 = (p2[2], p2[3]) if norm else (None, None)
        H1, H2 = int(W1.shape[0]), int(W2.shape[0])
        H1p, H2r = ops.round_up(H1, 32), ops.round_up(H2, 8)
        dg1 = db1n = dg2 = db2n = None
        if ctx.fused:
            xin, Fin, PQ, mask = ctx.saved
            N, dev = int(xin.shape[0]), xin.device
            adt = ops.act_dtype(mode)
            g_out = gout.contiguous().to(adt)
            dW2, db2 = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, g_out, mask, act=act1)      # also records the h > 0 bits
            dPQ = torch.empty((N, 2 * H1p), dtype=adt, device=dev)
            dpre = torch.empty((max(g.rows, 1), H1p), dtype=dt, device=dev)
            ops.edgeconv_bwd(mode, g, PQ, H1p, H2, g_out, mask, ops.pack_weight(W2.t().contiguous(), [H2], dt, 32), dpre,
                             dPQ[:, :H1p], act=act1, H1=H1)
            ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
        else:
            xin, Fin, pre1, a1, st1, z2, st2, aux = ctx.saved
            N, dev = int(xin.shape[0]), xin.device
            ic, jc = ops.edge_rows(g)
            grows = ops.slot_reduce_bwd(gout.contiguous().to(torch.float32), H2, g, aggr, aux, cpad=H2r)
            dz2, dg2, db2n = ops.rownorm_act_bwd(grows, z2, H2, act2, ln2[0], ln2[1], st2, valid=jc, cpad=H2r)
            dW2, db2 = ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
            da1 = ops.linear_fwd(mode, _ksegs([(dz2, H2)]), ops.pack_weight(W2.t(), [H2], dt, ku), H1, out_cols=H1p)
            dpre1, dg1, db1n = ops.rownorm_act_bwd(da1, pre1, H1, act1, ln1[0], ln1[1], st1, valid=jc, cpad=H1p)
            dPQ = torch.empty((N, 2 * H1p), dtype=torch.float32, device=dev)
            dPQ[:, :H1p] = ops.slot_sum(dpre1, H1p, g)
            ops.edgeconv_dq_gather(ops.MODE_F32, g, dpre1, H1p, dPQ[:, H1p:])
        dWpq, dbpq = ops.linear_wgrad(mode, dPQ, 2 * H1p, _ksegs([(xin, Fin)]), with_bias=True)
        dWpq = dWpq[:, :Fin]
        dWp, dWq = dWpq[:H1], dWpq[H1p:H1p + H1]
        grads: List[Optional[Tensor]] = [None] * len(params)
        grads[0] = torch.cat([dWp, dWq - dWp], dim=1)
        grads[1] = dbpq[:H1]
        grads[step] = dW2[:, :H1]
        grads[step + 1] = db2
        if norm:
            grads[2], grads[3], grads[step + 2], grads[step + 3] = dg1, db1n, dg2, db2n
        dx = None
        if ctx.needs_input_grad[1]:
            Wa, Wb = W1[:, :Fin], W1[:, Fin:]
            WpqT = torch.zeros((Fin, 2 * H1p), dtype=torch.float32, device=dev)
            WpqT[:, :H1] = (Wa - Wb).t()
            WpqT[:, H1p:H1p + H1] = Wb.t()
            dx = ops.linear_fwd(mode, [(dPQ, 2 * H1p)], ops.pack_weight(WpqT, [2 * H1p], dt, ku), Fin,
                                out_cols=ops.round_up(Fin, 8))[:, :Fin]
        return (None, dx) + tuple(grads)


class DynEdgeConv(torch.nn.Module):
    """Stand-alone dynamical edge convolution (``models/components/layers.py:20-69``): PyG ``EdgeConv`` with
    ``aggr`` in add / mean / max (reference default "max") followed by a k-NN re-clustering on
    ``features_subset`` of the new features.  ``nn`` must be ``Linear, [LayerNorm], act, Linear, [LayerNorm], act``
    with act in ReLU / GELU / LeakyReLU / Identity.  ``aggr="add"`` with ReLU or LeakyReLU after both layers and no
    LayerNorm runs on the fused edge kernels (``gn_edgeconv_fwd`` / ``gn_edgeconv_leaky_fwd`` and their backward), everything
    else on the unfused kernels (``csrc/generic.hip``).

    ``forward(x, edge_index, batch)`` accepts a ``[2, E]`` ``edge_index`` (grouped by target, in-degree
    <= nb_neighbors + 1) or a :class:`ops.NeighbourTable`; it returns ``(x', table)`` where ``table.edge_index()``
    materialises the PyG tensor the reference returns."""

    def __init__(self, nn: torch.nn.Module, aggr: str = "max", nb_neighbors: int = 8,
                 features_subset: Optional[Union[Sequence[int], slice]] = None, **kwargs: Any):
        super().__init__()
        if features_subset is None:
            features_subset = slice(None)
        assert isinstance(features_subset, (list, slice))
        if aggr not in ops.AGGR_CODES:
            raise ValueError(f"aggr {aggr!r} not supported")
        self.nn = nn
        self.aggr = aggr
        self.nb_neighbors = nb_neighbors
        self.features_subset = features_subset
        self._compute_mode = ops.MODE_BF16
        mods = list(nn) if isinstance(nn, torch.nn.Sequential) else None
        lin = [m for m in (mods or []) if isinstance(m, torch.nn.Linear)]
        norms = [m for m in (mods or []) if isinstance(m, torch.nn.LayerNorm)]
        acts = [m for m in (mods or []) if type(m) in _ACT_NAMES]
        if mods is None or len(lin) != 2 or len(acts) != 2 or len(norms) not in (0, 2) or \
                len(mods) != 4 + len(norms) or any(isinstance(m, torch.nn.LeakyReLU) and m.negative_slope != 0.01 for m in acts):
            raise NotImplementedError("graphnet_amd.DynEdgeConv: nn must be Linear, [LayerNorm], act, Linear, [LayerNorm], act "
                                      "(act: ReLU / GELU / LeakyReLU(0.01) / Identity); there is no fallback")
        self._lin, self._norms = lin, norms
        self._acts = (_ACT_NAMES[type(acts[0])], _ACT_NAMES[type(acts[1])])

    def set_backend(self, dtype: Optional[str] = None, fused: Optional[bool] = None) -> "DynEdgeConv":
        """``fused`` (default on): add aggregation with ReLU / LeakyReLU MLPs on the fused edge kernels."""
        if dtype is not None:
            self._compute_mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
        if fused is not None:
            self._fused = bool(fused)
        return self

    def forward(self, x: Tensor, edge_index: Any, batch: Optional[Tensor] = None):
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.DynEdgeConv runs on an MI355X (HIP) device only")
        N = int(x.shape[0])
        table = edge_index if isinstance(edge_index, ops.NeighbourTable) else \
            ops.table_from_edge_index(edge_index, N, self.nb_neighbors)
        params: List[Tensor] = []
        for i, lin in enumerate(self._lin):
            params += [lin.weight, lin.bias]
            if self._norms:
                params += [self._norms[i].weight, self._norms[i].bias]
        cfg = {"mode": self._compute_mode, "graph": table, "aggr": self.aggr, "norm": bool(self._norms), "acts": self._acts,
               "fused": getattr(self, "_fused", True)}
        out = _EdgeConvFunction.apply(cfg, x.to(torch.float32), *params)
        # re-cluster (layers.py:63-67)
        if batch is None:
            batch = torch.zeros(N, dtype=torch.int64, device=x.device)
        B = int(batch.max().item()) + 1 if N else 0
        ptr = torch.zeros(B + 1, dtype=torch.int32, device=x.device)
        ptr[1:] = torch.cumsum(torch.bincount(batch.to(torch.int64), minlength=B), 0).to(torch.int32)
        cols = _subset_cols(self.features_subset, int(out.shape[1]))
        if len(cols) > 8:
            raise NotImplementedError("graphnet_amd.DynEdgeConv: the k-NN kernel takes at most 8 coordinate columns")
        new_table = ops.knn_graph(out.detach(), cols, batch.to(torch.int32), ptr, self.nb_neighbors)
        return out, new_table
