"""Readable restatement of ``DeepIce`` for the tests (no product code): the reference's dense, padded formulation
(``models/gnn/icemix.py``, ``components/layers.py:200-596``, ``components/embedding.py``) on the CPU.

* the batch is padded to ``[B, L, .]`` and the spacetime bias is formed as ``[B, L, L, head_size]``;
* ``torch.nn.MultiheadAttention`` and ``torch.nn.LayerNorm`` themselves are used; module attribute names equal the
  reference's, so the state-dict keys do;
* the modules run in whatever dtype they are cast to (``.double()`` for the reference values, fp32 for the error a plain
  fp32 evaluation makes).  Two things do not follow that dtype: the frequency tables are the fp32 tables of the reference
  (formed on the host, then cast), and the pair argument ``a`` of the spacetime bias follows the CONTRACT of
  ``include/graphnet_amd.h`` - fp32, one rounding per operation, in a fixed order - and is then cast;
* :func:`attention_core` is the factored form the device kernel computes (``O``, ``U``), :func:`dense_rel_attention` the
  reference's form with the materialised bias; ``tests/test_deepice_host.py`` pins that the two agree.
"""
import math

import torch
import torch.nn as nn


def frequencies(dim, n_freq=10000.0):
    """The ``dim / 2`` frequencies of ``SinusoidalPosEmb(dim)`` in fp32, the reference's operations in their order."""
    half_dim = dim / 2
    emb = torch.log(torch.tensor([n_freq], dtype=torch.float32)) / half_dim
    return torch.exp(torch.arange(half_dim) * (-emb))


def sin_emb(x, dim):
    """``[sin(x f) | cos(x f)]`` appended to the shape of ``x``, in the dtype of ``x``."""
    arg = x.unsqueeze(-1) * frequencies(dim).to(x.dtype)
    return torch.cat((torch.sin(arg), torch.cos(arg)), dim=-1)


def pair_argument(x0):
    """``a[..., i, j] = 1024 clip(sign(ds) sqrt|ds|, -4, 4)`` for pulses ``x0[..., L, >= 4]`` (x, y, z, time), fp32 with one
    rounding per operation: ``ds = ((dx^2 + dy^2) + dz^2) - (dt 18)^2``, differences ``i - j``."""
    x0 = x0.to(torch.float32)
    factor = 3e4 / 500 * 3e-1
    assert factor == 18.0
    d = x0[..., :, None, :4] - x0[..., None, :, :4]
    dx2, dy2, dz2 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1], d[..., 2] * d[..., 2]
    dt = d[..., 3] * torch.tensor(factor, dtype=torch.float32)
    ds = ((dx2 + dy2) + dz2) - dt * dt
    # the fp32 square root of the contract is the correctly rounded one.  torch.sqrt on a CPU fp32 tensor is not (this build:
    # 0.7 % of random inputs one ulp off, and one ulp of d is up to 4.9e-4 rad in the sine argument), so it is taken in
    # double and rounded once: 53 >= 2 * 24 + 2 bits make that double rounding exact for a square root
    dist = torch.sign(ds) * torch.sqrt(torch.abs(ds).double()).to(torch.float32)
    return 1024 * dist.clip(-4, 4)


def _heads(t, H):
    """``[..., L, H dh] -> [..., H, L, dh]``."""
    return t.reshape(*t.shape[:-1], H, -1).transpose(-3, -2)


def attention_core(q, k, v, qp, s, H, mask=None):
    """The factored biased attention.  ``q, k, v, qp``: ``[..., L, H dh]``, ``s``: ``[..., L, L, dh]`` (the embedding of the
    pair argument), ``mask`` ``[..., L, L]`` additive.  Scores ``q k / sqrt(dh) + qp . s``; returns
    ``O = sum_j a_ij v_j`` and ``U = sum_j a_ij s_ij``, both ``[..., L, H dh]``."""
    qh, kh, vh, ph = _heads(q, H), _heads(k, H), _heads(v, H), _heads(qp, H)
    dh = qh.shape[-1]
    att = (qh * dh ** -0.5) @ kh.transpose(-1, -2) + torch.einsum("...hic,...ijc->...hij", ph, s)
    if mask is not None:
        att = att + mask.unsqueeze(-3)
    att = att.softmax(-1)
    O = att @ vh
    U = torch.einsum("...hij,...ijc->...hic", att, s)
    return O.transpose(-3, -2).flatten(-2), U.transpose(-3, -2).flatten(-2)


def dense_rel_attention(q, k, v, R, H, mask=None):
    """``Attention_rel`` between its projections, with the bias tensor ``R [..., L, L, dh]`` (or None) materialised."""
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    qh = qh * qh.shape[-1] ** -0.5
    att = qh @ kh.transpose(-1, -2)
    if R is not None:
        att = att + torch.einsum("...hic,...ijc->...hij", qh, R)
    if mask is not None:
        att = att + mask.unsqueeze(-3)
    att = att.softmax(-1)
    out = (att @ vh).transpose(-3, -2)
    if R is not None:
        out = out + torch.einsum("...hij,...ijc->...ihc", att, R)
    return out.flatten(-2)


def factored_rel_attention(q, k, v, s, W, b, H, mask=None):
    """The same through :func:`attention_core`: ``q' = W^T q~`` in, ``O + U W^T + b`` out."""
    dh = W.shape[0]
    qp = ((_heads(q, H) * dh ** -0.5) @ W).transpose(-3, -2).flatten(-2)
    O, U = attention_core(q, k, v, qp, s, H, mask)
    out = _heads(O, H) + _heads(U, H) @ W.t() + b
    return out.transpose(-3, -2).flatten(-2)


class SinusoidalPosEmb(nn.Module):
    def __init__(self, dim=16, n_freq=10000, scaled=False):
        super().__init__()
        self.scale = nn.Parameter(torch.ones(1) * dim ** -0.5) if scaled else 1.0
        self.dim = dim

    def forward(self, x):
        return sin_emb(x, self.dim) * self.scale


class FourierEncoder(nn.Module):
    def __init__(self, seq_length=128, mlp_dim=None, output_dim=384, scaled=False, n_features=6):
        super().__init__()
        self.sin_emb = SinusoidalPosEmb(dim=seq_length, scaled=scaled)
        self.sin_emb2 = SinusoidalPosEmb(dim=seq_length // 2, scaled=scaled)
        if n_features < 4:
            raise ValueError("x, y, z and time are required")
        if n_features >= 6:
            self.aux_emb = nn.Embedding(2, seq_length // 2)
            hidden_dim = 6 * seq_length
        else:
            hidden_dim = int((n_features + 0.5) * seq_length)
        mlp_dim = mlp_dim or hidden_dim
        self.mlp = nn.Sequential(nn.Linear(hidden_dim, mlp_dim), nn.LayerNorm(mlp_dim), nn.GELU(), nn.Linear(mlp_dim, output_dim))
        self.n_features = n_features

    def forward(self, x, n_pulses):
        """``x [B, L, F]`` padded with zeros, ``n_pulses [B]``."""
        L = x.shape[1]
        parts = [self.sin_emb(4096 * x[:, :, :3]).flatten(-2)]
        if self.n_features >= 5:
            parts.append(self.sin_emb(1024 * x[:, :, 4]))
        parts.append(self.sin_emb(4096 * x[:, :, 3]))
        if self.n_features >= 6:
            parts.append(self.aux_emb(x[:, :, 5].long()))
        length = torch.log10(n_pulses.to(x.dtype))
        parts.append(self.sin_emb2(length).unsqueeze(1).expand(-1, L, -1))
        return self.mlp(torch.cat(parts, -1))


class SpacetimeEncoder(nn.Module):
    def __init__(self, seq_length=32):
        super().__init__()
        self.sin_emb = SinusoidalPosEmb(dim=seq_length)
        self.projection = nn.Linear(seq_length, seq_length)

    def embedding(self, x0):
        """``s [B, L, L, seq_length]`` in the dtype of the projection, from the fp32 pair argument."""
        return self.sin_emb(pair_argument(x0).to(self.projection.weight.dtype))

    def forward(self, x0):
        return self.projection(self.embedding(x0))


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.input_projection = nn.Linear(in_features, hidden_features or in_features)
        self.activation = nn.GELU()
        self.output_projection = nn.Linear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        return self.output_projection(self.activation(self.input_projection(x)))


class Attention_rel(nn.Module):
    def __init__(self, input_dim, num_heads=8):
        super().__init__()
        self.num_heads = num_heads
        self.proj_q = nn.Linear(input_dim, input_dim, bias=False)
        self.proj_k = nn.Linear(input_dim, input_dim, bias=False)
        self.proj_v = nn.Linear(input_dim, input_dim, bias=False)
        self.proj = nn.Linear(input_dim, input_dim)

    def forward(self, x, real, rel_pos_bias=None):
        """``real [B, L]`` bool.  The reference adds ``min(m_i, m_j)`` of the 0 / -inf padding mask, reset to 0 where both are
        padding: -inf exactly where one of the two rows is a pulse and the other is padding."""
        mask = torch.zeros(real.shape[0], real.shape[1], real.shape[1], dtype=x.dtype)
        mask[real[:, :, None] != real[:, None, :]] = -math.inf
        return self.proj(dense_rel_attention(self.proj_q(x), self.proj_k(x), self.proj_v(x), rel_pos_bias, self.num_heads, mask))


class Block_rel(nn.Module):
    def __init__(self, input_dim, num_heads, mlp_ratio=4.0):
        super().__init__()
        self.norm1 = nn.LayerNorm(input_dim)
        self.attn = Attention_rel(input_dim, num_heads)
        self.norm2 = nn.LayerNorm(input_dim)
        self.mlp = Mlp(input_dim, int(input_dim * mlp_ratio))

    def forward(self, x, real, rel_pos_bias=None):
        x = x + self.attn(self.norm1(x), real, rel_pos_bias)
        return x + self.mlp(self.norm2(x))


class Block(nn.Module):
    def __init__(self, input_dim, num_heads, mlp_ratio=4.0, init_values=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(input_dim)
        self.attn = nn.MultiheadAttention(input_dim, num_heads, dropout=0.0, batch_first=True)
        self.norm2 = nn.LayerNorm(input_dim)
        self.mlp = Mlp(input_dim, int(input_dim * mlp_ratio))
        self.gamma_1 = nn.Parameter(init_values * torch.ones(input_dim))
        self.gamma_2 = nn.Parameter(init_values * torch.ones(input_dim))

    def forward(self, x, key_padding_mask):
        xn = self.norm1(x)
        x = x + self.gamma_1 * self.attn(xn, xn, xn, key_padding_mask=key_padding_mask, need_weights=False)[0]
        return x + self.gamma_2 * self.mlp(self.norm2(x))


def pad(x, batch):
    """``x [N, F]``, sorted ``batch [N]`` -> (``[B, L, F]`` zero padded, ``real [B, L]`` bool, ``n [B]``)."""
    n = torch.bincount(batch)
    B, L = int(n.shape[0]), int(n.max())
    real = torch.arange(L)[None, :] < n[:, None]
    out = torch.zeros(B, L, x.shape[1], dtype=x.dtype)
    out[real] = x
    return out, real, n


class DeepIce(nn.Module):
    def __init__(self, hidden_dim=384, mlp_ratio=4, seq_length=192, depth=12, head_size=32, depth_rel=4, n_rel=1,
                 scaled_emb=False, include_dynedge=False, dynedge_args=None, n_features=6):
        super().__init__()
        H = hidden_dim // head_size
        self.fourier_ext = FourierEncoder(seq_length, None, hidden_dim // 2 if include_dynedge else hidden_dim, scaled_emb,
                                          n_features)
        self.rel_pos = SpacetimeEncoder(head_size)
        self.sandwich = nn.ModuleList([Block_rel(hidden_dim, H) for _ in range(depth_rel)])
        self.cls_token = nn.Linear(hidden_dim, 1, bias=False)
        self.blocks = nn.ModuleList([Block(hidden_dim, H, mlp_ratio, init_values=1) for _ in range(depth)])
        self.n_rel = n_rel
        self.include_dynedge = include_dynedge
        if include_dynedge:
            from oracle.dynedge_oracle import DynEdgeOracle
            if dynedge_args is None:
                dynedge_args = dict(nb_inputs=9, nb_neighbours=9, post_processing_layer_sizes=[336, hidden_dim // 2],
                                    dynedge_layer_sizes=[(128, 256), (336, 256), (336, 256), (336, 256)],
                                    global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True,
                                    skip_readout=True)
            self.dyn_edge = DynEdgeOracle(**dynedge_args)

    def forward(self, x, batch, edge_index=None, forced_edges=None):
        """``x [N, F]`` fp32 pulses (x, y, z, time, charge, auxiliary, ...), ``batch [N]`` sorted -> ``[B, hidden_dim]`` in the
        modules' dtype.  ``edge_index`` / ``forced_edges``: the graphs of the embedded DynEdge (teacher forcing)."""
        dtype = self.cls_token.weight.dtype
        x0, real, n = pad(x.to(torch.float32), batch)
        h = self.fourier_ext(x0.to(dtype), n)
        rel_pos_bias = self.rel_pos(x0)
        if self.include_dynedge:
            g = self.dyn_edge(x.to(dtype), edge_index, batch, n.to(dtype), forced_edges=forced_edges)
            gp = torch.zeros(h.shape[0], h.shape[1], g.shape[1], dtype=dtype)
            gp[real] = g.to(dtype)
            h = torch.cat([h, gp], 2)
        for i, blk in enumerate(self.sandwich):
            h = blk(h, real, rel_pos_bias)
            if i + 1 == self.n_rel:
                rel_pos_bias = None
        B = h.shape[0]
        real = torch.cat([torch.ones(B, 1, dtype=torch.bool), real], 1)
        key_padding_mask = torch.zeros(real.shape, dtype=dtype)
        key_padding_mask[~real] = -math.inf
        h = torch.cat([self.cls_token.weight.unsqueeze(0).expand(B, -1, -1), h], 1)
        for blk in self.blocks:
            h = blk(h, key_padding_mask)
        return h[:, 0]
