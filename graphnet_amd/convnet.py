"""graphnet_amd/convnet.py — ``ConvNet`` (``models/gnn/convnet.py`` of the reference) on the HIP kernels.

Three ``TAGConv(., ., K=2)`` layers on the loader's static graph, each followed by a leaky ReLU and a
``global_add_pool | global_max_pool`` per event, then ``BatchNorm1d``, five ``Linear + leaky_relu + Dropout`` and ``out``
on the pooled ``[B, 6 * nb_intermediate]`` rows.  Same constructor, same attribute names, so the reference's state-dict
keys hold (``conv{1,2,3}.lins.{0,1,2}.weight``, ``conv{1,2,3}.bias``, ``batchnorm1.*``, ``linear{1..5}.*``, ``out.*``).

Kernels (``csrc/tagconv.hip``): a layer's forward is ``h1 = P x`` (``gn_tag_propagate``) and the fused
``gn_tagconv_fwd`` (gathers ``h2 = P h1`` into the LDS operand, one MFMA GEMM over ``[x | h1 | h2]``, bias and leaky ReLU
on the accumulators).  The backward is Horner's scheme: ``[g0 | g1 | g2] = dpre [W0 | W1 | W2]`` in one GEMM,
``dx = g0 + P^T (g1 + P^T g2)`` on ``gn_tag_propagate_t``, the weight gradient in one three-segment GEMM.  The table,
``dis = deg^-1/2`` and the reverse lists are built once per forward for all three layers; pooling runs on
``gn_segment_pool_fwd`` / ``_bwd``.  The per-event layers after the pooling stay torch device ops.
"""
from __future__ import annotations

from typing import Any, Optional, Union

import torch
from torch import Tensor

from . import ops
from .gnn import GNN, _maybe, _no_radial_record
from .tito import _wt

_POOLS = ["sum", "max"]            # global_add_pool | global_max_pool: the reference's column order


class _TAGConvFunction(torch.autograd.Function):
    """``leaky_relu(x W0^T + (P x) W1^T + (P P x) W2^T + b, 0.01)``; widths are multiples of 32 here."""

    @staticmethod
    def forward(ctx, cfg: dict, x: Tensor, W0: Tensor, W1: Tensor, W2: Tensor, bias: Optional[Tensor]) -> Tensor:  # type: ignore[override]
        mode, g, dis = cfg["mode"], cfg["graph"], cfg["dis"]
        Cout, Cin = int(W0.shape[0]), int(W0.shape[1])
        x = x.contiguous()
        h1 = ops.tag_propagate(x, Cin, g, dis)
        b = None if bias is None else bias.detach().contiguous()
        out, h2 = ops.tagconv_fwd(mode, x, h1, g, dis, ops.tagconv_pack((W0, W1, W2), mode), b, Cin, Cout)
        ctx.cfg = cfg
        ctx.save_for_backward(x, h1, h2, out, W0, W1, W2)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        x, h1, h2, out, W0, W1, W2 = ctx.saved_tensors
        mode, g, dis = ctx.cfg["mode"], ctx.cfg["graph"], ctx.cfg["dis"]
        Cout, Cin = int(W0.shape[0]), int(W0.shape[1])
        dpre = ops.tag_dpre(gout.contiguous().to(torch.float32), out, Cout)
        dW, db = ops.linear_wgrad(mode, dpre, Cout, [(x, Cin), (h1, Cin), (h2, Cin)], with_bias=True)
        dx = None
        if ctx.needs_input_grad[1]:
            WT = torch.cat([W0, W1, W2], dim=1).t()                       # [3 Cin, Cout]: G = dpre [W0 | W1 | W2]
            G = ops.linear_fwd(mode, [(dpre, Cout)], _wt(mode, WT, [Cout]), 3 * Cin)
            g1 = ops.tag_propagate_t(G[:, 2 * Cin:], Cin, g, dis, add=G[:, Cin:2 * Cin])
            dx = ops.tag_propagate_t(g1, Cin, g, dis, add=G[:, :Cin])
        return None, dx, dW[:, :Cin], dW[:, Cin:2 * Cin], dW[:, 2 * Cin:], (db if ctx.has_bias else None)


class _SumMaxPoolFunction(torch.autograd.Function):
    """``[global_add_pool | global_max_pool]`` per event on the fused segment-pool kernels (argmax backward)."""

    @staticmethod
    def forward(ctx, x: Tensor, ptr: Tensor, batch: Tensor) -> Tensor:  # type: ignore[override]
        C = int(x.shape[1])
        pooled, ctx.amin, ctx.amax = ops.segment_pool_fwd(x, C, ptr, _POOLS)
        ctx.ptr, ctx.batch, ctx.shape = ptr, batch, (int(x.shape[0]), C)
        return pooled

    @staticmethod
    def backward(ctx, gout: Tensor):  # type: ignore[override]
        N, C = ctx.shape
        dx = ops.segment_pool_bwd(gout.contiguous().to(torch.float32), C, ctx.ptr, ctx.batch, N, _POOLS, ctx.amin, ctx.amax, None)
        return dx, None, None


class TAGConv(torch.nn.Module):
    """``torch_geometric.nn.TAGConv`` for ``K = 2`` with ``gcn_norm`` (no self loops), fused with the leaky ReLU that follows it
    in ``ConvNet`` (``fused_leaky_relu``; the kernels have no other epilogue).  Parameters ``lins.{k}.weight`` and ``bias``."""

    def __init__(self, in_channels: int, out_channels: int, K: int = 2, bias: bool = True, normalize: bool = True):
        super().__init__()
        if K != 2 or not normalize:
            raise NotImplementedError("graphnet_amd.TAGConv: the HIP kernels cover K = 2 with normalize = True only")
        cin_p = ops.round_up(in_channels, 32)
        if cin_p > 256 or out_channels % 32 or not 32 <= out_channels <= 256:
            raise NotImplementedError("graphnet_amd.TAGConv: in_channels <= 256 (zero-padded to a multiple of 32) and "
                                      f"out_channels a multiple of 32 in [32, 256]; got {in_channels}, {out_channels}")
        self.in_channels, self.out_channels, self.K, self.normalize = in_channels, out_channels, K, normalize
        self.lins = torch.nn.ModuleList([torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(K + 1)])
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)
        self._compute_mode = ops.MODE_BF16

    def forward(self, x: Tensor, graph: Union[Tensor, ops.NeighbourTable], dis: Optional[Tensor] = None,
                mode: Optional[int] = None) -> Tensor:
        """``leaky_relu(TAGConv(x, graph), 0.01)``; ``graph``: ``edge_index`` or a neighbour table (then ``dis`` may be
        passed along, so several layers share one ``ops.tag_norm``)."""
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.TAGConv runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        if not isinstance(graph, ops.NeighbourTable):
            graph = ops.table_from_edge_index(graph, int(x.shape[0]), 8)
        if graph.K > 32:
            raise NotImplementedError("graphnet_amd.TAGConv: in-degrees above 33 are outside the kernels' envelope")
        if dis is None:
            dis = ops.tag_norm(graph)
        pad = ops.round_up(self.in_channels, 32) - self.in_channels
        x = x.to(torch.float32)
        W = [lin.weight for lin in self.lins]
        if pad:                                       # zero columns: the gradient of the real ones is unchanged
            x = torch.nn.functional.pad(x, (0, pad))
            W = [torch.nn.functional.pad(w, (0, pad)) for w in W]
        cfg = {"mode": self._compute_mode if mode is None else mode, "graph": graph, "dis": dis}
        return _TAGConvFunction.apply(cfg, x, W[0], W[1], W[2], self.bias)


class ConvNet(GNN):
    """ConvNet (convolutional network) model on MI355X; constructor as ``gnn/convnet.py:19-62``."""

    def __init__(self, nb_inputs: int, nb_outputs: int, nb_intermediate: int = 128, dropout_ratio: float = 0.3):
        if nb_intermediate % 32 or not 32 <= nb_intermediate <= 256:
            raise NotImplementedError("graphnet_amd.ConvNet: nb_intermediate must be a multiple of 32 in [32, 256] "
                                      f"(got {nb_intermediate}); there is no fallback path")
        super().__init__(nb_inputs, nb_outputs)
        self.nb_intermediate = nb_intermediate
        self.nb_intermediate2 = 6 * nb_intermediate
        self.conv1 = TAGConv(nb_inputs, nb_intermediate, 2)
        self.conv2 = TAGConv(nb_intermediate, nb_intermediate, 2)
        self.conv3 = TAGConv(nb_intermediate, nb_intermediate, 2)
        self.batchnorm1 = torch.nn.BatchNorm1d(self.nb_intermediate2)
        for l in range(1, 6):
            setattr(self, f"linear{l}", torch.nn.Linear(self.nb_intermediate2, self.nb_intermediate2))
            setattr(self, f"drop{l}", torch.nn.Dropout(dropout_ratio))
        self.out = torch.nn.Linear(self.nb_intermediate2, nb_outputs)
        self._compute_mode = ops.MODE_BF16
        self._nb_neighbours = 8

    def set_backend(self, *, dtype: str = "bf16", nb_neighbours: Optional[int] = None) -> "ConvNet":
        """``dtype``: compute type of the MFMA GEMMs; ``nb_neighbours``: table width an ``edge_index`` is first tried with."""
        self._compute_mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
        if nb_neighbours is not None:
            self._nb_neighbours = nb_neighbours
        return self

    def forward(self, data: Any) -> Tensor:
        """Apply learnable forward pass (``convnet.py:64-117``)."""
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.ConvNet runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        N = int(x.shape[0])
        ptr = _maybe(data, "ptr")
        if ptr is None:
            B = int(data.n_pulses.shape[0]) if _maybe(data, "n_pulses") is not None else int(data.batch.max().item()) + 1
            ptr = torch.zeros(B + 1, dtype=torch.int64, device=x.device)
            ptr[1:] = torch.cumsum(torch.bincount(data.batch, minlength=B), 0)
        ptr32 = ptr.to(torch.int32)
        batch = _maybe(data, "batch")
        batch32 = batch.to(torch.int32) if batch is not None else ops.ptr_to_batch(ptr32, N)
        table = _maybe(data, "nbr_table")
        if not isinstance(table, ops.NeighbourTable):
            ei = _maybe(data, "edge_index")
            if ei is None:
                raise ValueError("graphnet_amd.ConvNet needs the loader's graph: data.edge_index or data.nbr_table")
            _no_radial_record(data, ei, type(self).__name__)
            table = ops.table_from_edge_index(ei, N, self._nb_neighbours)
        dis = ops.tag_norm(table)                       # once for the three layers; the reverse lists are built on first use
        pooled = []
        for conv in (self.conv1, self.conv2, self.conv3):
            x = conv(x, table, dis, self._compute_mode)
            pooled.append(_SumMaxPoolFunction.apply(x, ptr32, batch32))
        x = self.batchnorm1(torch.cat(pooled, dim=1))
        for l in range(1, 6):
            x = getattr(self, f"drop{l}")(torch.nn.functional.leaky_relu(getattr(self, f"linear{l}")(x)))
        return self.out(x)
