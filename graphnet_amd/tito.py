"""graphnet_amd/tito.py — ``DynEdgeTITO`` on the HIP kernels.

Mirrors ``/root/reference/src/graphnet/models/gnn/dynedge_kaggle_tito.py`` (ctor l.32-138, layers l.140-196, forward
l.236-268) and ``models/components/layers.py:72-197`` (``EdgeConvTito``, ``DynTrans``): same constructor
arguments, same sub-module names — hence the same state-dict keys, Lightning-checkpoint compatible.

What runs where
  * ``EdgeConvTito`` (message ``nn([x_i, x_j - x_i, x_j])``, max aggregation, static edges): the per-node split
    ``W1 [x_i | x_j-x_i | x_j] = (Wa - Wb) x_i + (Wb + Wc) x_j`` turns the first Linear into one MFMA GEMM over
    nodes; LeakyReLU / second Linear / arg-routed max on the edge-row kernels of ``csrc/generic.hip``.
  * the transformer encoder layer: in/out projections and the 2048-wide FFN on the MFMA GEMM kernels with fused
    bias / relu / residual-accumulate epilogues, LayerNorms on the row kernels, and the attention itself on
    ``csrc/attn.hip`` — ragged, every pulse attends to its own event, no ``to_dense_batch`` padding.
  * dropout (``TransformerEncoderLayer``'s default 0.1, as in the reference): stateless counter-based keep rule
    (``gn_dropout``), applied to the attention probabilities inside the attention kernels and to the three
    element-wise sites by one small kernel; nothing is stored, the backward recomputes the decisions.  The random
    stream differs from torch's Philox stream by construction (as it does between any two torch devices).
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import ops
from .gnn import GNN, _ksegs, _maybe, _no_radial_record

_DT_PARAMS = 18   # tensors per DynTrans layer, see DynTrans.kernel_params


def _wt(mode: int, W: Tensor, widths: Sequence[int]) -> Tensor:
    return ops.pack_weight(W, widths, ops.mode_dtype(mode), ops.gemm_kunit(mode))


class _DynTransFunction(torch.autograd.Function):
    """One ``DynTrans`` layer (``layers.py:117-197``) as a single autograd node."""

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, *p: Tensor) -> Tensor:  # type: ignore[override]
        (W1, b1, W2, b2, g0, be0, Win, bin_, Wout, bout, Wl1, bl1, Wl2, bl2, g1, be1, g2, be2) = p
        mode, g, H = cfg["mode"], cfg["graph"], cfg["n_head"]
        ptr, plan = cfg["ptr"], cfg["plan"]
        dev = x.device
        N, Fin = int(x.shape[0]), int(x.shape[1])
        H1, d = int(W1.shape[0]), int(W2.shape[0])
        H1p, dr = ops.round_up(H1, 32), ops.round_up(d, 8)
        if d % 32 or d > 512:
            raise NotImplementedError("graphnet_amd.DynTrans: d_model must be a multiple of 32, at most 512")
        xin = torch.zeros((N, ops.round_up(Fin, 32)), dtype=torch.float32, device=dev)
        xin[:, :Fin] = x
        # --- EdgeConvTito: P = (Wa - Wb) x + b1, Q = (Wb + Wc) x
        Wa, Wb, Wc = W1[:, :Fin], W1[:, Fin:2 * Fin], W1[:, 2 * Fin:]
        Wpq = torch.zeros((2 * H1p, Fin), dtype=torch.float32, device=dev)
        Wpq[:H1] = Wa - Wb
        Wpq[H1p:H1p + H1] = Wb + Wc
        bpq = torch.zeros(2 * H1p, dtype=torch.float32, device=dev)
        bpq[:H1] = b1
        lp = mode == ops.MODE_BF16                  # GEMM-only operands are produced in bf16 (weights-stationary GEMM)
        residual = Fin == d                                             # layers.py:183-186
        gx = cfg.get("graph_exact")
        fused = gx is not None and ops.edgeconv_max_supported(mode, gx, H1p, d)
        if fused:
            # fused EdgeConvTito (csrc/edgeconv_v2.hip, variant 1): gather + leaky relu + second Linear on the matrix
            # core + max / arg-slot epilogue in one persistent kernel; no edge-row tensor reaches HBM
            PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), _wt(mode, Wpq, [Fin]), 2 * H1p, bias=bpq, out_lowp=True)
            conv16, esaved = ops.edgeconv_max_fwd(gx, PQ, H1p, ops.pack_weight(W2, [H1], torch.bfloat16), b2.contiguous(), d)
            r = torch.empty((N, d), dtype=torch.float32, device=dev)
            ops.dropout(conv16, 0, 0, res=x.contiguous() if residual else None, out=r)     # r = (x +) conv, fp32
            a1 = z2 = aux = None
            if cfg.get("arg_log") is not None:          # trace: the max aggregation's routing decisions
                cfg["arg_log"].append(ops.edgeconv_max_arg_rank(gx, esaved, H1p, d))
        else:
            PQ = ops.linear_fwd(mode, _ksegs([(xin, Fin)]), _wt(mode, Wpq, [Fin]), 2 * H1p, bias=bpq)
            ic, jc = ops.edge_rows(g)
            # leaky relu preserves the sign: a1 is produced by the gather itself and its derivative is read off a1's
            # sign in the backward (no pre-activation tensor); the second one commutes with the max aggregation
            a1 = ops.edge_gather_pre(PQ, H1p, ic, jc, act="leaky_relu", lowp=lp)
            z2 = ops.linear_fwd(mode, [(a1, H1p)], _wt(mode, W2, [H1]), d, bias=b2.contiguous(), out_cols=dr)
            conv, aux = ops.slot_reduce(z2, d, g, "max", post_act="leaky_relu")
            if cfg.get("arg_log") is not None:
                cfg["arg_log"].append(ops.argrow_to_rank(g, aux[1], d))
            r = conv.add_(x) if residual else conv
            conv16 = esaved = None
            PQ = None
        y0, st0 = ops.rownorm_act_fwd(r, d, "identity", g0, be0, lowp="both" if lp else "no")      # self.norm1
        y0, y0g = y0 if lp else (y0, y0)            # fp32 for the residual stream, bf16 copy for the GEMMs
        # --- TransformerEncoderLayer, norm_first=False
        lowp = ops.attention_lowp(mode, d, H)       # bf16 qkv / attention output, matrix-core attention kernels
        qkv = ops.linear_fwd(mode, _ksegs([(y0g, d)]), _wt(mode, Win, [d]), 3 * d, bias=bin_.contiguous(), out_lowp=lowp)
        drop = cfg.get("drop")                      # None, or (thresh, [seed_attn, seed_1, seed_ffn, seed_2])
        th = drop[0] if drop else 0
        # dropout on the attention probabilities: the matrix-core kernels save their keep decisions as bits (both
        # orientations) so that the two backward passes read them instead of re-evaluating the hash
        dlay = cfg.get("drop_layout") if drop and lowp else None
        dbits = None
        if dlay is not None:
            att, lse2, dbits = ops.attention_fwd_saved(qkv, H, ptr, plan, (drop[1][0], th), dlay)
        else:
            att, lse2 = ops.attention_fwd(qkv, H, ptr, plan, drop=(drop[1][0], th) if drop else None)
        if drop:                                    # x + dropout1(self_attn(x))
            proj = ops.linear_fwd(mode, _ksegs([(att, d)]), _wt(mode, Wout, [d]), d, bias=bout.contiguous())
            z1 = ops.dropout(proj, drop[1][1], th, res=y0)
        else:
            z1 = y0.clone()
            ops.linear_fwd(mode, _ksegs([(att, d)]), _wt(mode, Wout, [d]), d, bias=bout.contiguous(), out=z1, accum=True)
        y1, st1 = ops.rownorm_act_fwd(z1, d, "identity", g1, be1, lowp="both" if lp else "no")
        y1, y1g = y1 if lp else (y1, y1)
        F = int(Wl1.shape[0])
        h = ops.linear_fwd(mode, _ksegs([(y1g, d)]), _wt(mode, Wl1, [d]), F, bias=bl1.contiguous(), relu=True,
                           out_lowp=mode == ops.MODE_BF16)     # the 2048-wide hidden layer is stored in the operand type
        if drop:                                    # x + dropout2(linear2(dropout(relu(linear1(x)))))
            ops.dropout(h, drop[1][2], th, out=h)
            f = ops.linear_fwd(mode, _ksegs([(h, F)]), _wt(mode, Wl2, [F]), d, bias=bl2.contiguous())
            z3 = ops.dropout(f, drop[1][3], th, res=y1)
        else:
            z3 = y1.clone()
            ops.linear_fwd(mode, _ksegs([(h, F)]), _wt(mode, Wl2, [F]), d, bias=bl2.contiguous(), out=z3, accum=True)
        y2, st2 = ops.rownorm_act_fwd(z3, d, "identity", g2, be2)
        ctx.cfg, ctx.p = cfg, p
        ctx.saved = (xin, Fin, a1, z2, aux, residual, r, st0, y0g, qkv, att, lse2, z1, st1, y1g, h, z3, st2)
        ctx.fused = (PQ, conv16, esaved) if fused else None
        ctx.dbits = dbits
        return y2

    @staticmethod
    def backward(ctx, gy: Tensor):  # type: ignore[override]
        cfg, p = ctx.cfg, ctx.p
        (W1, b1, W2, b2, g0, be0, Win, bin_, Wout, bout, Wl1, bl1, Wl2, bl2, g1, be1, g2, be2) = p
        (xin, Fin, a1, z2, aux, residual, r, st0, y0, qkv, att, lse2, z1, st1, y1, h, z3, st2) = ctx.saved
        mode, g, H = cfg["mode"], cfg["graph"], cfg["n_head"]
        ptr, plan = cfg["ptr"], cfg["plan"]
        dev = xin.device
        N = int(xin.shape[0])
        H1, d, F = int(W1.shape[0]), int(W2.shape[0]), int(Wl1.shape[0])
        H1p, dr = ops.round_up(H1, 32), ops.round_up(d, 8)
        grads: List[Optional[Tensor]] = [None] * _DT_PARAMS
        gy = gy.contiguous().to(torch.float32)
        # norm2, FFN
        drop = cfg.get("drop")
        th = drop[0] if drop else 0
        lp = mode == ops.MODE_BF16
        dz3, grads[16], grads[17] = ops.rownorm_act_bwd(gy, z3, d, "identity", g2, be2, st2,
                                                        lowp="both" if lp and not drop else "no")
        dz3, dz3g = dz3 if lp and not drop else (dz3, dz3)      # fp32: residual gradient; bf16 copy: GEMM operand
        df = ops.dropout(dz3, drop[1][3], th, out=torch.empty_like(dz3, dtype=ops.mode_dtype(mode))) if drop else dz3g
        grads[12], grads[13] = ops.linear_wgrad(mode, df, d, _ksegs([(h, F)]), with_bias=True)
        dh = ops.linear_fwd(mode, _ksegs([(df, d)]), _wt(mode, Wl2.t(), [d]), F, gate=h, out_lowp=h.dtype == torch.bfloat16)
        # dropout on the hidden layer, backward: h is the POST-dropout activation, so the gate (h > 0) above is already
        # closed on every dropped unit; what is left of dropout's backward is the factor 1 / (1 - p) on the kept ones.
        # Both consumers of dh are linear in it: the factor goes into the weight gradient and into the packed Wl1^T
        # (two tiny tensors) instead of a pass over the [N, 2048] tensor with a hash per element.
        inv = 1.0 / (1.0 - th / 4294967296.0) if drop else 1.0
        grads[10], grads[11] = ops.linear_wgrad(mode, dh, F, _ksegs([(y1, d)]), with_bias=True)
        if drop:
            grads[10] = grads[10] * inv
            grads[11] = grads[11] * inv
        ops.linear_fwd(mode, _ksegs([(dh, F)]), _wt(mode, Wl1.t() * inv if drop else Wl1.t(), [F]), d, out=dz3, accum=True)      # dy1
        # norm1, attention
        dz1, grads[14], grads[15] = ops.rownorm_act_bwd(dz3, z1, d, "identity", g1, be1, st1,
                                                        lowp="both" if lp and not drop else "no")
        dz1, dz1g = dz1 if lp and not drop else (dz1, dz1)
        dproj = ops.dropout(dz1, drop[1][1], th, out=torch.empty_like(dz1, dtype=ops.mode_dtype(mode))) if drop else dz1g
        grads[8], grads[9] = ops.linear_wgrad(mode, dproj, d, _ksegs([(att, d)]), with_bias=True)
        datt = ops.linear_fwd(mode, _ksegs([(dproj, d)]), _wt(mode, Wout.t(), [d]), d, out_lowp=qkv.dtype == torch.bfloat16)
        if ctx.dbits is not None:
            dqkv = ops.attention_bwd_saved(qkv, H, ptr, plan, att, lse2, datt, th, ctx.dbits, cfg["drop_layout"])
        else:
            dqkv = ops.attention_bwd(qkv, H, ptr, plan, att, lse2, datt, drop=(drop[1][0], th) if drop else None)
        grads[6], grads[7] = ops.linear_wgrad(mode, dqkv, 3 * d, _ksegs([(y0, d)]), with_bias=True)
        ops.linear_fwd(mode, _ksegs([(dqkv, 3 * d)]), _wt(mode, Win.t(), [3 * d]), d, out=dz1, accum=True)  # dy0
        # DynTrans.norm1
        dres, grads[4], grads[5] = ops.rownorm_act_bwd(dz1, r, d, "identity", g0, be0, st0)
        # EdgeConvTito
        if ctx.fused is not None:
            PQ, conv16, esaved = ctx.fused
            gx = cfg["graph_exact"]
            # d(loss)/d(max) = dres * leaky'(out): read off the sign of the stored (bf16) output
            gmax, _, _ = ops.rownorm_act_bwd(dres, conv16, d, "leaky_relu", cpad=d, lowp="only")
            grads[2], grads[3] = ops.edgeconv_max_dw2(gx, PQ, H1p, H1, d, gmax, esaved)      # also records h > 0 bits
            dPQ = torch.empty((N, 2 * H1p), dtype=torch.bfloat16, device=dev)
            dpre1 = torch.empty((max(gx.rows, 1), H1p), dtype=torch.bfloat16, device=dev)
            ops.edgeconv_max_bwd(gx, H1p, d, gmax, esaved, ops.pack_weight(W2.t(), [d], torch.bfloat16), dpre1, dPQ[:, :H1p])
            ops.edgeconv_dq_gather(ops.MODE_BF16, gx, dpre1, H1p, dPQ[:, H1p:])
        else:
            ic, jc = ops.edge_rows(g)
            dz2, _, _ = ops.rownorm_act_bwd(dres, z2, d, "leaky_relu", valid=jc, gidx=ic, argrow=aux[1], cpad=dr,
                                            lowp="only" if lp else "no")        # max routing + leaky' in one pass
            dW2, grads[3] = ops.linear_wgrad(mode, dz2, d, [(a1, H1p)], with_bias=True)
            grads[2] = dW2[:, :H1]
            da1 = ops.linear_fwd(mode, _ksegs([(dz2, d)]), _wt(mode, W2.t(), [d]), H1, out_cols=H1p)
            dpre1, _, _ = ops.rownorm_act_bwd(da1, a1, H1, "leaky_relu", valid=jc, cpad=H1p)
            dPQ = torch.empty((N, 2 * H1p), dtype=torch.float32, device=dev)
            dPQ[:, :H1p] = ops.slot_sum(dpre1, H1p, g)
            ops.edgeconv_dq_gather(ops.MODE_F32, g, dpre1, H1p, dPQ[:, H1p:])
        dWpq, dbpq = ops.linear_wgrad(mode, dPQ, 2 * H1p, _ksegs([(xin, Fin)]), with_bias=True)
        dWpq = dWpq[:, :Fin]
        dWp, dWq = dWpq[:H1], dWpq[H1p:H1p + H1]
        grads[0] = torch.cat([dWp, dWq - dWp, dWq], dim=1)               # d/dWa, d/dWb, d/dWc
        grads[1] = dbpq[:H1]
        dx = None
        if ctx.needs_input_grad[1]:
            Wa, Wb, Wc = W1[:, :Fin], W1[:, Fin:2 * Fin], W1[:, 2 * Fin:]
            WpqT = torch.zeros((Fin, 2 * H1p), dtype=torch.float32, device=dev)
            WpqT[:, :H1] = (Wa - Wb).t()
            WpqT[:, H1p:H1p + H1] = (Wb + Wc).t()
            if residual:        # Fin == d: the residual branch's gradient is the accumulate target
                dx = ops.linear_fwd(mode, [(dPQ, 2 * H1p)], _wt(mode, WpqT, [2 * H1p]), Fin, out=dres, accum=True)
            else:
                dx = ops.linear_fwd(mode, [(dPQ, 2 * H1p)], _wt(mode, WpqT, [2 * H1p]), Fin,
                                    out_cols=ops.round_up(Fin, 8))[:, :Fin]
        return (None, dx) + tuple(grads)


class _GlobalsFunction(torch.autograd.Function):
    """``ops.graph_globals`` for node features that carry a gradient (``RNN_TITO``: the GRU states are columns of ``x``):
    the per-event feature means pass it on (``dynedge_kaggle_tito.py:214-234``: ``scatter_mean`` is differentiable); the
    homophily columns compare for equality and ``log10(n_pulses)`` is data."""

    @staticmethod
    def forward(ctx, x: Tensor, ptr: Tensor, batch: Tensor, table: Any, n_pulses: Tensor) -> Tensor:  # type: ignore[override]
        ctx.ptr, ctx.batch, ctx.shape = ptr, batch, (int(x.shape[0]), int(x.shape[1]))
        return ops.graph_globals(x, ptr, table, n_pulses)

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        N, F = ctx.shape
        dx = ops.segment_pool_bwd(gout[:, :F].to(torch.float32), F, ctx.ptr, ctx.batch, N, ["mean"], None, None, None)
        return dx, None, None, None, None


class _PostPoolFunction(torch.autograd.Function):
    """Post-processing MLP (Linear + LeakyReLU per layer, ``dynedge_kaggle_tito.py:160-174``) followed by the
    global pooling (``l.198-212``).  ``params``: W, b per layer."""

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, *params: Tensor) -> Tensor:  # type: ignore[override]
        mode = cfg["mode"]
        segs = [(x.contiguous(), int(x.shape[1]))]
        zs = []
        for t in range(len(params) // 2):
            W, b = params[2 * t], params[2 * t + 1]
            P_ = int(W.shape[0])
            z = ops.linear_fwd(mode, _ksegs(segs), _wt(mode, W, [segs[0][1]]), P_, bias=b.contiguous(),
                               out_cols=ops.round_up(P_, 8))
            y, _ = ops.rownorm_act_fwd(z, P_, "leaky_relu", cpad=ops.round_up(P_, 8))
            zs.append(z)
            segs = [(y, P_)]
        y_last, P = segs[0]
        ctx.cfg, ctx.params, ctx.x, ctx.zs = cfg, params, x, zs
        cfg["post"] = y_last[:, :P] if cfg.get("want_trace") else None
        pooled, ctx.amin, ctx.amax = ops.segment_pool_fwd(y_last, P, cfg["ptr"], cfg["pools"])
        cfg["pool_arg"] = {"min": ctx.amin, "max": ctx.amax} if cfg.get("want_trace") else None    # routing of min / max pooling
        return pooled

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        cfg, params, x, zs = ctx.cfg, ctx.params, ctx.x, ctx.zs
        mode = cfg["mode"]
        N = int(x.shape[0])
        nl = len(params) // 2
        P = int(params[-2].shape[0]) if nl else int(x.shape[1])
        gy = ops.segment_pool_bwd(gout.contiguous().to(torch.float32), P, cfg["ptr"], cfg["batch"], N, cfg["pools"],
                                  ctx.amin, ctx.amax, None)
        grads: List[Optional[Tensor]] = [None] * len(params)
        for t in reversed(range(nl)):
            W = params[2 * t]
            Pt, Pin = int(W.shape[0]), int(W.shape[1])
            # dz is only ever a GEMM operand (weight gradient, input gradient): bf16 in bf16 mode, as the MFMA would
            # round it anyway - and bf16 dY carries the bias gradient as a ones block of the same GEMM
            dz, _, _ = ops.rownorm_act_bwd(gy.contiguous(), zs[t], Pt, "leaky_relu", cpad=ops.round_up(Pt, 8),
                                           lowp="only" if mode == ops.MODE_BF16 else "no")
            if t > 0:
                yprev, _ = ops.rownorm_act_fwd(zs[t - 1], Pin, "leaky_relu", cpad=ops.round_up(Pin, 8))
                in_segs = [(yprev, Pin)]
            else:
                in_segs = [(x.contiguous(), Pin)]
            dW, grads[2 * t + 1] = ops.linear_wgrad(mode, dz, Pt, _ksegs(in_segs), with_bias=True)
            grads[2 * t] = dW[:, :Pin]
            gy = ops.linear_fwd(mode, _ksegs([(dz, Pt)]), _wt(mode, W.t(), [Pt]), Pin, out_cols=ops.round_up(Pin, 8))
        return (None, gy[:, :int(x.shape[1])]) + tuple(grads)


class DynTrans(torch.nn.Module):
    """Parameter holder + launcher of one ``DynTrans`` layer; attribute names as in ``layers.py:117-164``."""

    def __init__(self, layer_sizes: Optional[List[int]] = None, aggr: str = "max",
                 features_subset: Any = None, n_head: int = 8, dropout: float = 0.1, **kwargs: Any):
        super().__init__()
        if features_subset is None:
            features_subset = slice(None)
        assert isinstance(features_subset, (list, slice))
        if aggr != "max":
            raise NotImplementedError("graphnet_amd.DynTrans: aggr must be 'max' (what DynEdgeTITO uses); no fallback")
        if layer_sizes is None:
            layer_sizes = [256, 256, 256]
        if len(layer_sizes) != 3:
            raise NotImplementedError("graphnet_amd.DynTrans: the edge MLP must have exactly two layers; no fallback")
        layers: List[torch.nn.Module] = []
        for ix, (nb_in, nb_out) in enumerate(zip(layer_sizes[:-1], layer_sizes[1:])):
            if ix == 0:
                nb_in *= 3
            layers.append(torch.nn.Linear(nb_in, nb_out))
            layers.append(torch.nn.LeakyReLU())
        d_model = layer_sizes[-1]
        self.nn = torch.nn.Sequential(*layers)
        self.features_subset = features_subset
        self.norm1 = torch.nn.LayerNorm(d_model, eps=1e-5)
        enc = torch.nn.TransformerEncoderLayer(d_model=d_model, nhead=n_head, batch_first=True, norm_first=False,
                                               dropout=dropout)
        self._transformer_encoder = torch.nn.TransformerEncoder(enc, num_layers=1)
        self._n_head = n_head
        self._dropout = dropout

    def kernel_params(self) -> List[Tensor]:
        e = self._transformer_encoder.layers[0]
        sa = e.self_attn
        return [self.nn[0].weight, self.nn[0].bias, self.nn[2].weight, self.nn[2].bias, self.norm1.weight, self.norm1.bias,
                sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias,
                e.linear1.weight, e.linear1.bias, e.linear2.weight, e.linear2.bias,
                e.norm1.weight, e.norm1.bias, e.norm2.weight, e.norm2.bias]

    def forward(self, x: Tensor, cfg: dict) -> Tensor:
        cfg = dict(cfg, n_head=self._n_head)
        if self.training and self._dropout > 0.0:
            # four independent streams per call: attention probabilities, dropout1, FFN dropout, dropout2
            # (torch.nn.MultiheadAttention / TransformerEncoderLayer); seeds come from torch's CPU generator, so
            # torch.manual_seed makes a run reproducible
            seeds = torch.randint(0, 2 ** 31 - 1, (4,)).tolist()
            cfg["drop"] = (ops.drop_thresh(self._dropout), seeds)
            if cfg.get("seed_log") is not None:
                cfg["seed_log"].append(seeds)
        return _DynTransFunction.apply(cfg, x, *self.kernel_params())


class DynEdgeTITO(GNN):
    """DynEdgeTITO (dynamical edge convolution with transformer) on MI355X.  Constructor as
    ``dynedge_kaggle_tito.py:32-59`` plus ``dropout`` (the rate the reference gets from torch's default)."""

    def __init__(self, nb_inputs: int, features_subset: Optional[List[int]] = None,
                 dyntrans_layer_sizes: Optional[List[Tuple[int, ...]]] = None,
                 global_pooling_schemes: List[str] = ["max"], use_global_features: bool = True,
                 use_post_processing_layers: bool = True, post_processing_layer_sizes: Optional[List[int]] = None,
                 readout_layer_sizes: Optional[List[int]] = None, n_head: int = 8, nb_neighbours: int = 8,
                 dropout: float = 0.1):
        if dyntrans_layer_sizes is None:
            dyntrans_layer_sizes = [(256, 256)] * 4
        assert isinstance(dyntrans_layer_sizes, list) and len(dyntrans_layer_sizes)
        dyntrans_layer_sizes = [tuple(s) for s in dyntrans_layer_sizes]
        assert all(len(s) > 0 and all(v > 0 for v in s) for s in dyntrans_layer_sizes)
        self._dyntrans_layer_sizes = dyntrans_layer_sizes
        self._post_processing_layer_sizes = post_processing_layer_sizes or [336, 256]
        self._readout_layer_sizes = readout_layer_sizes or [256, 128]
        if isinstance(global_pooling_schemes, str):
            global_pooling_schemes = [global_pooling_schemes]
        assert global_pooling_schemes, "No global pooling schemes were request, so cannot add global variables after pooling."
        for s in global_pooling_schemes:
            assert s in ops.POOL_CODES, f"Global pooling scheme {s} not supported."
        self._global_pooling_schemes = list(global_pooling_schemes)
        super().__init__(nb_inputs, self._readout_layer_sizes[-1])
        self._activation = torch.nn.LeakyReLU()
        self._nb_inputs = nb_inputs
        self._nb_global_variables = 5 + nb_inputs
        self._nb_neighbours = nb_neighbours
        self._features_subset = features_subset or [0, 1, 2, 3]
        self._use_global_features = use_global_features
        self._use_post_processing_layers = use_post_processing_layers
        self._n_head = n_head
        self._compute_mode = ops.MODE_BF16
        self._knn_strict = False
        self._graph_columns = [0, 1, 2]
        # layers (dynedge_kaggle_tito.py:140-196)
        self._conv_layers = torch.nn.ModuleList()
        lat = nb_inputs
        for sizes in dyntrans_layer_sizes:
            self._conv_layers.append(DynTrans([lat] + list(sizes), aggr="max", features_subset=self._features_subset,
                                              n_head=n_head, dropout=dropout))
            lat = sizes[-1]
        if use_post_processing_layers:
            mods: List[torch.nn.Module] = []
            ls = [lat] + list(self._post_processing_layer_sizes)
            for a, b in zip(ls[:-1], ls[1:]):
                mods += [torch.nn.Linear(a, b), self._activation]
            self._post_processing = torch.nn.Sequential(*mods)
            lat = ls[-1]
        lat = lat * len(self._global_pooling_schemes) + (self._nb_global_variables if use_global_features else 0)
        mods = []
        ls = [lat] + list(self._readout_layer_sizes)
        for a, b in zip(ls[:-1], ls[1:]):
            mods += [torch.nn.Linear(a, b), self._activation]
        self._readout = torch.nn.Sequential(*mods)

    def set_backend(self, *, dtype: str = "bf16", knn_mode: str = "compat",
                    graph_columns: Optional[Sequence[int]] = None) -> "DynEdgeTITO":
        """``dtype``: "fp32" (exact-f32 MFMA, parity mode) or "bf16" (bf16 MFMA operands, fp32 accumulate and
        storage).  ``graph_columns``: coordinates of the k-NN built on device when the batch has no edges."""
        self._compute_mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
        self._knn_strict = {"compat": False, "strict": True}[knn_mode]
        if graph_columns is not None:
            self._graph_columns = list(graph_columns)
        return self

    def forward(self, data: Any, return_trace: bool = False) -> Tensor:
        """Apply learnable forward pass (``dynedge_kaggle_tito.py:236-268``)."""
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.DynEdgeTITO runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        x = x.to(torch.float32)
        N = int(x.shape[0])
        n_pulses = data.n_pulses.to(torch.int32)
        ptr = _maybe(data, "ptr")
        if ptr is None:
            ptr = torch.zeros(n_pulses.shape[0] + 1, dtype=torch.int64, device=x.device)
            ptr[1:] = torch.cumsum(torch.bincount(data.batch, minlength=n_pulses.shape[0]), 0)
        ptr32 = ptr.to(torch.int32)
        batch = _maybe(data, "batch")
        batch32 = batch.to(torch.int32) if batch is not None else ops.ptr_to_batch(ptr32, N)
        table = _maybe(data, "nbr_table")
        if not isinstance(table, ops.NeighbourTable):
            ei = _maybe(data, "edge_index")
            _no_radial_record(data, ei, type(self).__name__)
            table = ops.table_from_edge_index(ei, N, self._nb_neighbours) if ei is not None else \
                ops.knn_graph(x, self._graph_columns, batch32, ptr32, self._nb_neighbours, strict=self._knn_strict)
        plan = ops.attention_plan(ptr32)
        if self._use_global_features and x.requires_grad:
            gv = _GlobalsFunction.apply(x, ptr32, batch32, table, n_pulses)
        else:
            gv = ops.graph_globals(x, ptr32, table, n_pulses) if self._use_global_features else None
        seed_log: List[List[int]] = []
        # static graph: one table without overflow rows for the fused EdgeConvTito kernels (bf16 mode), shared by all
        # DynTrans layers; its reverse lists are built once
        exact = ops.exact_table(table) if self._compute_mode == ops.MODE_BF16 and getattr(self, "_fused_edges", True) else None
        if exact is not None and exact.K > 16:
            exact = None
        arg_log: List[Tensor] = []
        cfg = {"mode": self._compute_mode, "graph": table, "graph_exact": exact, "ptr": ptr32, "batch": batch32, "plan": plan,
               "seed_log": seed_log if return_trace else None, "arg_log": arg_log if return_trace else None}
        if self.training and self._compute_mode == ops.MODE_BF16 and getattr(self, "_save_drop_bits", True) and \
                any(getattr(l, "_dropout", 0.0) > 0.0 for l in self._conv_layers):
            cfg["drop_layout"] = ops.attention_drop_layout(ptr32)
        conv_out = []
        for conv in self._conv_layers:
            x = conv(x, cfg)
            conv_out.append(x)
        pcfg = {"mode": self._compute_mode, "ptr": ptr32, "batch": batch32, "pools": self._global_pooling_schemes,
                "want_trace": return_trace}
        post_params: List[Tensor] = []
        if self._use_post_processing_layers:
            for m in self._post_processing:
                if isinstance(m, torch.nn.Linear):
                    post_params += [m.weight, m.bias]
        pooled = _PostPoolFunction.apply(pcfg, x, *post_params)
        out = torch.cat([pooled, gv], dim=1) if self._use_global_features else pooled
        out = self._readout(out)
        if return_trace:
            return out, {"conv_out": conv_out, "post": pcfg.get("post"), "pooled": pooled, "global_variables": gv,
                         "graph": table, "dropout_seeds": seed_log, "max_arg_rank": arg_log, "pool_arg": pcfg.get("pool_arg")}
        return out
