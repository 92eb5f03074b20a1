"""``DeepIce`` (the IceMix transformer of the Kaggle "Neutrinos in Deep Ice" solution) on the ragged attention kernels.

Mirror of ``models/gnn/icemix.py``, ``models/components/layers.py:200-596`` and ``models/components/embedding.py``: the same
constructor signatures, defaults and sub-module names, hence the same state-dict keys.  The reference pads the batch to
``[B, L, d]``, materialises the spacetime bias as ``[B, L, L, head_size]`` fp32 and contracts it twice per layer.  Here the
batch stays ragged (``x``, ``ptr``) and neither tensor exists:

* blocks with the spacetime bias run on ``csrc/attn_rel.hip``.  With ``s_ij`` the sinusoidal embedding of the clipped
  4-distance and ``R_ij = W s_ij + b`` (``rel_pos.projection``), ``q~ . k + q~ . R_ij = q~ . k + (W^T q~) . s_ij + const`` and
  ``sum_j a_ij (v_j + R_ij) = O_i + W U_i + b`` with ``U_i = sum_j a_ij s_ij``: the kernel takes ``q, k, v`` and ``q' = W^T q~``,
  recomputes ``s_ij`` per pair and returns ``O`` and ``U``; ``W`` and ``b`` stay in two small GEMMs with plain autograd;
* blocks without it (the rest of ``sandwich``, and ``blocks`` with the cls row of every event) run on ``csrc/attn.hip``;
* the reference's mask arithmetic reduces, for real pulses, to "keys of the own event only", which is what both kernels do.

Linear, LayerNorm and GELU run on torch's device ops with plain autograd (bf16 mode: bf16 GEMM operands, fp32 residual
stream and LayerNorm).  All dropout and drop-path rates of ``DeepIce`` are 0 in the reference; no dropout path is built and
a non-zero rate raises.  There is no fallback: outside the kernels' envelope the forward raises.
"""
from __future__ import annotations

import math
from typing import Any, Dict, Optional, Set

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import ops
from .gnn import GNN, DynEdge, _maybe
from .model import Model


class _RaggedAttentionFunction(torch.autograd.Function):
    """Plain ragged attention (``ops.attention_fwd`` / ``attention_bwd``), no dropout: qkv ``[N, 3 d]`` -> ``[N, d]``."""

    @staticmethod
    def forward(ctx, qkv: Tensor, n_head: int, ptr: Tensor, plan: Tensor) -> Tensor:  # type: ignore[override]
        qkv = qkv.contiguous()
        out, lse2 = ops.attention_fwd(qkv, n_head, ptr, plan)
        ctx.save_for_backward(qkv, out, lse2, ptr, plan)
        ctx.n_head = n_head
        return out

    @staticmethod
    def backward(ctx, dout: Tensor):  # type: ignore[override]
        qkv, out, lse2, ptr, plan = ctx.saved_tensors
        return ops.attention_bwd(qkv, ctx.n_head, ptr, plan, out, lse2, dout.contiguous().to(qkv.dtype)), None, None, None


class _RelAttentionFunction(torch.autograd.Function):
    """Ragged attention with the spacetime bias recomputed per pair (``ops.rel_attention_fwd`` / ``rel_attention_bwd``):
    (qkv ``[N, 3 d]``, qp ``[N, d]``) -> (out, u), both ``[N, d]``; ``xt`` and ``freq`` are data."""

    @staticmethod
    def forward(ctx, qkv: Tensor, qp: Tensor, xt: Tensor, freq: Tensor, n_head: int, ptr: Tensor, plan: Tensor):  # type: ignore[override]
        qkv, qp = qkv.contiguous(), qp.contiguous()
        out, u, lse2 = ops.rel_attention_fwd(qkv, qp, xt, freq, n_head, ptr, plan)
        ctx.save_for_backward(qkv, qp, xt, freq, ptr, plan, out, u, lse2)
        ctx.n_head = n_head
        return out, u

    @staticmethod
    def backward(ctx, dout: Tensor, du: Tensor):  # type: ignore[override]
        qkv, qp, xt, freq, ptr, plan, out, u, lse2 = ctx.saved_tensors
        dqkv, dqp = ops.rel_attention_bwd(qkv, qp, xt, freq, ctx.n_head, ptr, plan, out, u, lse2,
                                          dout.contiguous().to(torch.float32), du.contiguous().to(torch.float32))
        return dqkv, dqp, None, None, None, None, None


def _linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], mode: int) -> Tensor:
    """``F.linear``; bf16 mode: bf16 operands and output (fp32 accumulation inside the GEMM)."""
    if mode == ops.MODE_BF16:
        return F.linear(x.to(torch.bfloat16), weight.to(torch.bfloat16), None if bias is None else bias.to(torch.bfloat16))
    return F.linear(x, weight, bias)


def _no_dropout(who: str, **rates: float) -> None:
    for name, p in rates.items():
        if p:
            raise NotImplementedError(f"graphnet_amd.{who}: {name}={p}: dropout is not built in these blocks "
                                      "(every rate of DeepIce is 0 in the reference)")


class SinusoidalPosEmb(Model):
    """``embedding.py:11-50``: ``[sin(x f_k) | cos(x f_k)] * scale``, ``f_k = n_freq^(-k / (dim / 2))``.  The frequency table
    is the reference's fp32 one, formed on the host; the products ``x f_k`` (up to ~5000 rad) are formed and reduced mod 2 pi
    in double, so the embedding is the exact function of the fp32 input rather than 2e-4 rad away from it."""

    def __init__(self, dim: int = 16, n_freq: int = 10000, scaled: bool = False):
        super().__init__()
        if dim % 2 != 0:
            raise ValueError(f"dim has to be even. Got: {dim}")
        self.scale = nn.Parameter(torch.ones(1) * dim ** -0.5) if scaled else 1.0
        self.dim = dim
        self.n_freq = torch.Tensor([n_freq])

    def frequencies(self, device: Any) -> Tensor:
        half_dim = self.dim / 2
        emb = torch.log(self.n_freq) / half_dim
        return torch.exp(torch.arange(half_dim) * (-emb)).to(device)

    def forward(self, x: Tensor) -> Tensor:
        arg = x.to(torch.float64).unsqueeze(-1) * self.frequencies(x.device).to(torch.float64)
        arg = torch.remainder(arg, 2.0 * math.pi).to(torch.float32)
        return torch.cat((torch.sin(arg), torch.cos(arg)), dim=-1) * self.scale


class FourierEncoder(Model):
    """``embedding.py:53-136`` on ragged rows: ``forward(x [N, >= n_features], seq_length [B], batch [N]) -> [N, output_dim]``.
    Columns: x, y, z, time, charge, auxiliary (the first four are mandatory)."""

    def __init__(self, seq_length: int = 128, mlp_dim: Optional[int] = None, output_dim: int = 384, scaled: bool = False,
                 n_features: int = 6):
        super().__init__()
        self.sin_emb = SinusoidalPosEmb(dim=seq_length, scaled=scaled)
        self.sin_emb2 = SinusoidalPosEmb(dim=seq_length // 2, scaled=scaled)
        if n_features < 4:
            raise ValueError(f"At least x, y, z and time of the DOM are required. Got only {n_features} features.")
        elif n_features >= 6:
            self.aux_emb = nn.Embedding(2, seq_length // 2)
            hidden_dim = 6 * seq_length
        else:
            hidden_dim = int((n_features + 0.5) * seq_length)
        if mlp_dim is None:
            mlp_dim = hidden_dim
        self.mlp = nn.Sequential(nn.Linear(hidden_dim, mlp_dim), nn.LayerNorm(mlp_dim), nn.GELU(), nn.Linear(mlp_dim, output_dim))
        self.n_features = n_features

    def forward(self, x: Tensor, seq_length: Tensor, batch: Tensor, mode: int = ops.MODE_F32) -> Tensor:
        N = int(x.shape[0])
        length = torch.log10(seq_length.to(dtype=x.dtype))
        embeddings = [self.sin_emb(4096 * x[:, :3]).reshape(N, -1)]              # position
        if self.n_features >= 5:
            embeddings.append(self.sin_emb(1024 * x[:, 4]))                      # charge
        embeddings.append(self.sin_emb(4096 * x[:, 3]))                          # time
        if self.n_features >= 6:
            embeddings.append(self.aux_emb(x[:, 5].long()))                      # auxiliary
        embeddings.append(self.sin_emb2(length)[batch])                          # log10 of the event's pulse count
        h = torch.cat(embeddings, -1)
        lin0, norm, act, lin1 = self.mlp
        h = _linear(h, lin0.weight, lin0.bias, mode).to(torch.float32)
        h = act(norm(h))
        return _linear(h, lin1.weight, lin1.bias, mode).to(torch.float32)


class SpacetimeEncoder(Model):
    """``embedding.py:139-175``: holds ``projection`` (``R_ij = W s_ij + b``) only.  Its ``[L, L, seq_length]`` output is never
    formed: the attention kernel recomputes ``s_ij`` per pair, ``Attention_rel`` applies ``W`` and ``b`` outside it."""

    def __init__(self, seq_length: int = 32):
        super().__init__()
        self.sin_emb = SinusoidalPosEmb(dim=seq_length)
        self.projection = nn.Linear(seq_length, seq_length)

    def forward(self, x: Tensor) -> Tensor:
        raise NotImplementedError("graphnet_amd.SpacetimeEncoder: the pair tensor is never materialised; pass the module to "
                                  "Attention_rel, which folds it into the attention kernel")


class DropPath(Model):
    """``layers.py:200-229``; identity at rate 0, the only rate ``DeepIce`` uses."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        _no_dropout("DropPath", drop_prob=drop_prob)
        self.drop_prob = drop_prob

    def forward(self, x: Tensor) -> Tensor:
        return x

    def extra_repr(self) -> str:
        return "p={}".format(self.drop_prob)


class Mlp(Model):
    """``layers.py:232-273``: Linear, activation, Linear."""

    def __init__(self, in_features: int, hidden_features: Optional[int] = None, out_features: Optional[int] = None,
                 activation: Any = nn.GELU, dropout_prob: float = 0.0):
        super().__init__()
        if in_features <= 0:
            raise ValueError(f"in_features must be greater than 0, got in_features {in_features} instead")
        _no_dropout("Mlp", dropout_prob=dropout_prob)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.input_projection = nn.Linear(in_features, hidden_features)
        self.activation = activation()
        self.output_projection = nn.Linear(hidden_features, out_features)
        self.dropout = nn.Dropout(dropout_prob)

    def forward(self, x: Tensor, mode: int = ops.MODE_F32) -> Tensor:
        h = self.activation(_linear(x, self.input_projection.weight, self.input_projection.bias, mode))
        return _linear(h, self.output_projection.weight, self.output_projection.bias, mode).to(torch.float32)


def _plain_attention(qkv: Tensor, n_head: int, cfg: Dict[str, Any]) -> Tensor:
    """Ragged attention over ``cfg['ptr']``: bf16 tensors on the matrix-core kernels where they exist, else exact fp32."""
    d = int(qkv.shape[1]) // 3
    if d % n_head or d // n_head not in (8, 16, 32, 64):
        raise NotImplementedError(f"ragged attention: head width {d / n_head:g} is not built (8, 16, 32 and 64 are); no fallback")
    lowp = ops.attention_lowp(cfg["mode"], d, n_head)
    qkv = qkv.to(torch.bfloat16 if lowp else torch.float32)
    return _RaggedAttentionFunction.apply(qkv, n_head, cfg["ptr"], cfg["plan"])


class Attention_rel(Model):
    """``layers.py:389-499`` on ragged rows.  ``forward(x [N, d], cfg, rel)``: ``rel`` is the ``SpacetimeEncoder`` whose bias
    the scores and values take, or None for plain attention; ``cfg`` holds ``ptr`` (int32), ``plan``, ``mode`` and, for the
    bias, ``xt`` ``[N, >= 4]`` (x, y, z, time) and ``freq``."""

    def __init__(self, input_dim: int, num_heads: int = 8, qkv_bias: bool = False, qk_scale: Optional[float] = None,
                 attn_drop: float = 0.0, proj_drop: float = 0.0, attn_head_dim: Optional[int] = None):
        if input_dim <= 0 or num_heads <= 0:
            raise ValueError(f"dim and num_heads must be greater than 0, got input_dim={input_dim} and num_heads={num_heads} instead")
        super().__init__()
        _no_dropout("Attention_rel", attn_drop=attn_drop, proj_drop=proj_drop)
        self.num_heads = num_heads
        head_dim = attn_head_dim or input_dim // num_heads
        all_head_dim = head_dim * self.num_heads
        if qk_scale is not None and qk_scale != head_dim ** -0.5:
            raise NotImplementedError("graphnet_amd.Attention_rel: the kernels scale the scores by head_dim^-0.5 only")
        self.scale = qk_scale or head_dim ** -0.5
        self.proj_q = nn.Linear(input_dim, all_head_dim, bias=False)
        self.proj_k = nn.Linear(input_dim, all_head_dim, bias=False)
        self.proj_v = nn.Linear(input_dim, all_head_dim, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(all_head_dim))
            self.v_bias = nn.Parameter(torch.zeros(all_head_dim))
        else:
            self.q_bias = None
            self.v_bias = None
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(all_head_dim, input_dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def forward(self, x: Tensor, cfg: Dict[str, Any], rel: Optional[SpacetimeEncoder] = None) -> Tensor:
        mode, H = cfg["mode"], self.num_heads
        N = int(x.shape[0])
        W = torch.cat([self.proj_q.weight, self.proj_k.weight, self.proj_v.weight], 0)
        b = None
        if self.q_bias is not None:
            b = torch.cat([self.q_bias, torch.zeros_like(self.q_bias), self.v_bias])
        qkv = _linear(x, W, b, mode)                                             # [N, 3 d] = Q | K | V
        d = int(qkv.shape[1]) // 3
        dh = d // H
        if rel is None:
            att = _plain_attention(qkv, H, cfg)
        else:
            if int(rel.projection.weight.shape[0]) != dh:
                raise ValueError(f"Attention_rel: the spacetime encoder is {rel.projection.weight.shape[0]} wide, the heads {dh}")
            if not ops.rel_attention_supported(dh):
                raise NotImplementedError(f"graphnet_amd.Attention_rel: the biased attention kernels are built for head width "
                                          f"32, not {dh}; there is no fallback")
            qkv = qkv.to(torch.float32)
            Wr, br = rel.projection.weight, rel.projection.bias                  # R_ij = Wr s_ij + br
            qp = torch.matmul(qkv[:, :d].reshape(N, H, dh) * self.scale, Wr).reshape(N, d)      # W^T q~ per head
            out, u = _RelAttentionFunction.apply(qkv, qp, cfg["xt"], cfg["freq"], H, cfg["ptr"], cfg["plan"])
            att = (out.reshape(N, H, dh) + torch.matmul(u.reshape(N, H, dh), Wr.t()) + br).reshape(N, d)
        return _linear(att, self.proj.weight, self.proj.bias, mode).to(torch.float32)


def _gammas(self: nn.Module, input_dim: int, init_values: Optional[float]) -> None:
    if init_values is not None:
        self.gamma_1 = nn.Parameter(init_values * torch.ones(input_dim), requires_grad=True)
        self.gamma_2 = nn.Parameter(init_values * torch.ones(input_dim), requires_grad=True)
    else:
        self.gamma_1, self.gamma_2 = None, None


class Block_rel(Model):
    """``layers.py:276-386`` (BEiTv2 block): ``x + attn(norm1 x)``, ``x + mlp(norm2 x)``, self attention only."""

    def __init__(self, input_dim: int, num_heads: int, mlp_ratio: float = 4.0, qkv_bias: bool = False,
                 qk_scale: Optional[float] = None, dropout: float = 0.0, attn_drop: float = 0.0, drop_path: float = 0.0,
                 init_values: Optional[float] = None, activation: Any = nn.GELU, norm_layer: Any = nn.LayerNorm,
                 attn_head_dim: Optional[int] = None):
        super().__init__()
        self.norm1 = norm_layer(input_dim)
        self.attn = Attention_rel(input_dim, num_heads, attn_drop=attn_drop, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                  attn_head_dim=attn_head_dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(input_dim)
        self.mlp = Mlp(in_features=input_dim, hidden_features=int(input_dim * mlp_ratio), activation=activation,
                       dropout_prob=dropout)
        _gammas(self, input_dim, init_values)

    def forward(self, x: Tensor, cfg: Dict[str, Any], rel: Optional[SpacetimeEncoder] = None) -> Tensor:
        a = self.attn(self.norm1(x), cfg, rel)
        x = x + (a if self.gamma_1 is None else self.gamma_1 * a)
        m = self.mlp(self.norm2(x), cfg["mode"])
        return x + (m if self.gamma_2 is None else self.gamma_2 * m)


class Block(Model):
    """``layers.py:502-596``: a ``nn.MultiheadAttention``-layout block (``attn.in_proj_weight`` ...); the module only holds
    the parameters, the attention runs on the ragged kernels."""

    def __init__(self, input_dim: int, num_heads: int, mlp_ratio: float = 4.0, dropout: float = 0.0, attn_drop: float = 0.0,
                 drop_path: float = 0.0, init_values: Optional[float] = None, activation: Any = nn.GELU,
                 norm_layer: Any = nn.LayerNorm):
        super().__init__()
        _no_dropout("Block", attn_drop=attn_drop)
        self.norm1 = norm_layer(input_dim)
        self.attn = nn.MultiheadAttention(input_dim, num_heads, dropout=attn_drop, batch_first=True)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(input_dim)
        self.mlp = Mlp(in_features=input_dim, hidden_features=int(input_dim * mlp_ratio), activation=activation,
                       dropout_prob=dropout)
        _gammas(self, input_dim, init_values)

    def forward(self, x: Tensor, cfg: Dict[str, Any]) -> Tensor:
        mode, sa = cfg["mode"], self.attn
        qkv = _linear(self.norm1(x), sa.in_proj_weight, sa.in_proj_bias, mode)
        a = _plain_attention(qkv, sa.num_heads, cfg)
        a = _linear(a, sa.out_proj.weight, sa.out_proj.bias, mode).to(torch.float32)
        x = x + (a if self.gamma_1 is None else self.gamma_1 * a)
        m = self.mlp(self.norm2(x), mode)
        return x + (m if self.gamma_2 is None else self.gamma_2 * m)


class DeepIce(GNN):
    """DeepIce on MI355X; constructor as ``icemix.py:34-47``.  Takes any ragged batch (``x``, ``ptr`` or ``batch``) whose first
    columns are x, y, z, time, charge, auxiliary (``n_features`` of them are used) and returns ``[B, hidden_dim]``."""

    def __init__(self, hidden_dim: int = 384, mlp_ratio: int = 4, seq_length: int = 192, depth: int = 12, head_size: int = 32,
                 depth_rel: int = 4, n_rel: int = 1, scaled_emb: bool = False, include_dynedge: bool = False,
                 dynedge_args: Dict[str, Any] = None, n_features: int = 6):
        super().__init__(seq_length, hidden_dim)
        if hidden_dim % head_size:
            raise ValueError(f"DeepIce: hidden_dim {hidden_dim} is not a multiple of head_size {head_size}")
        fourier_out_dim = hidden_dim // 2 if include_dynedge else hidden_dim
        self.fourier_ext = FourierEncoder(seq_length=seq_length, mlp_dim=None, output_dim=fourier_out_dim, scaled=scaled_emb,
                                          n_features=n_features)
        self.rel_pos = SpacetimeEncoder(head_size)
        self.sandwich = nn.ModuleList([Block_rel(input_dim=hidden_dim, num_heads=hidden_dim // head_size)
                                       for _ in range(depth_rel)])
        self.cls_token = nn.Linear(hidden_dim, 1, bias=False)
        self.blocks = nn.ModuleList([Block(input_dim=hidden_dim, num_heads=hidden_dim // head_size, mlp_ratio=mlp_ratio,
                                           drop_path=0.0, init_values=1) for _ in range(depth)])
        self.n_rel = n_rel
        if include_dynedge and dynedge_args is None:
            self.dyn_edge = DynEdge(nb_inputs=9, nb_neighbours=9, post_processing_layer_sizes=[336, hidden_dim // 2],
                                    dynedge_layer_sizes=[(128, 256), (336, 256), (336, 256), (336, 256)],
                                    global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True,
                                    skip_readout=True)
        elif include_dynedge:
            args = dict(dynedge_args)
            if args.get("dynedge_layer_sizes") is not None:                      # (YAML has no tuples)
                args["dynedge_layer_sizes"] = [tuple(s) for s in args["dynedge_layer_sizes"]]
            self.dyn_edge = DynEdge(**args)
        self.include_dynedge = include_dynedge
        self._head_size = head_size
        self._compute_mode = ops.MODE_BF16

    def no_weight_decay(self) -> Set:
        """cls_token should not be subject to weight decay during training."""
        return {"cls_token"}

    def set_backend(self, *, dtype: str = "bf16", knn_mode: str = "compat") -> "DeepIce":
        """``dtype``: "fp32" (parity mode) or "bf16" (bf16 GEMM operands and plain attention on the matrix core; the residual
        stream, LayerNorm and the biased attention kernel stay fp32).  Passed on to the embedded ``DynEdge``."""
        self._compute_mode = {"fp32": ops.MODE_F32, "f32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
        if self.include_dynedge:
            self.dyn_edge.set_backend(dtype=dtype, knn_mode=knn_mode)
        return self

    def forward(self, data: Any) -> Tensor:
        """Apply learnable forward pass (``icemix.py:127-167``)."""
        x = data.x
        if not x.is_cuda:
            raise RuntimeError("graphnet_amd.DeepIce runs on an MI355X (HIP) device only; move the batch to 'cuda'.")
        x = x.to(torch.float32)
        N, dev, mode = int(x.shape[0]), x.device, self._compute_mode
        if int(x.shape[1]) < self.fourier_ext.n_features:
            raise ValueError(f"DeepIce(n_features={self.fourier_ext.n_features}): the batch has {int(x.shape[1])} columns")
        if not ops.rel_attention_supported(self._head_size):
            raise NotImplementedError(f"graphnet_amd.DeepIce: head_size {self._head_size} is outside the biased attention "
                                      "kernels' envelope (32); there is no fallback")
        ptr = _maybe(data, "ptr")
        batch = _maybe(data, "batch")
        if ptr is None:
            nb = int(batch.max().item()) + 1 if N else 0
            ptr = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
            ptr[1:] = torch.cumsum(torch.bincount(batch, minlength=nb), 0)
        ptr = ptr.to(torch.int64)
        ptr32 = ptr.to(torch.int32)
        B = int(ptr.shape[0]) - 1
        batch = ops.ptr_to_batch(ptr32, N).to(torch.int64) if batch is None else batch.to(torch.int64)
        h = self.fourier_ext(x, ptr[1:] - ptr[:-1], batch, mode)
        if self.include_dynedge:
            h = torch.cat([h, self.dyn_edge(data).to(torch.float32)], 1)
        cfg = {"mode": mode, "ptr": ptr32, "plan": ops.attention_plan(ptr32), "xt": x[:, :4].contiguous(),
               "freq": self.rel_pos.sin_emb.frequencies(dev).contiguous()}
        rel: Optional[SpacetimeEncoder] = self.rel_pos
        for i, blk in enumerate(self.sandwich):
            h = blk(h, cfg, rel)
            if i + 1 == self.n_rel:                 # (n_rel = 0 or n_rel > depth_rel: every block keeps the bias, as in the reference)
                rel = None
        # one cls row in front of every event: row r of the new batch is row take[r] of [cls | h]
        ev = torch.arange(B, device=dev)
        pos_cls = ptr[:-1] + ev
        pos_pulse = torch.arange(N, device=dev) + batch + 1
        take = torch.empty(N + B, dtype=torch.int64, device=dev)
        take[pos_cls] = 0
        take[pos_pulse] = 1 + torch.arange(N, device=dev)
        h = torch.cat([self.cls_token.weight, h], 0)[take]
        ptr_cls = (ptr + torch.arange(B + 1, device=dev)).to(torch.int32)
        cfg = {"mode": mode, "ptr": ptr_cls, "plan": ops.attention_plan(ptr_cls)}
        for blk in self.blocks:
            h = blk(h, cfg)
        return h[pos_cls]
