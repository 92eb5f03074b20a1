#!/usr/bin/env python3
"""The LayerNorm + GELU edge MLP of the DynEdge that DeepIce embeds, fused (csrc/edgeconv_norm.hip) against unfused
(csrc/generic.hip), on synthetic IceCube-86 events with k = 9: one (336, 256) layer forward and forward + backward at the
kernel level, and the four-layer embedded DynEdge as a training step (fwd + bwd + AdamW).  The two paths alternate in one
session; every figure is the median of 5 windows of device-event time after a warm-up, with the peak of
torch.cuda.max_memory_allocated over the path's windows.

usage: run_norm_edgeconv.py [B] [fp32|bf16] [reps per window]"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphnet_amd as g                                              # noqa: E402
from graphnet_amd import ops                                          # noqa: E402
from graphnet_amd.synthetic import synthetic_icecube86_raw            # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
dtype = sys.argv[2] if len(sys.argv) > 2 else "bf16"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
dt = ops.mode_dtype(mode)
K, H1, H1p, H2 = 9, 336, 352, 256
torch.manual_seed(0)

raw, ptr, _ = synthetic_icecube86_raw(B, seed=5)
n = ptr[1:] - ptr[:-1]
x = torch.randn(int(ptr[-1]), 9)
x[:, :4] = torch.from_numpy(raw[:, :4].copy())
x[:, :3] /= 500.0
batch = g.Batch(x=x.to("cuda"))
batch.ptr = torch.from_numpy(ptr).to(torch.int64).to("cuda")
batch.batch = torch.repeat_interleave(torch.arange(B), torch.from_numpy(n)).to("cuda")
batch.n_pulses = torch.from_numpy(n).to(torch.int32).to("cuda")
N = int(x.shape[0])


def alternate(fns, windows=5, warm=2):
    """{name: (median ms per call, peak GiB)} with the callables taking turns window by window."""
    times, peak = {k: [] for k in fns}, {k: 0.0 for k in fns}
    for w in range(warm + windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            z.record()
            torch.cuda.synchronize()
            if w >= warm:
                times[name].append(a.elapsed_time(z) / reps)
                peak[name] = max(peak[name], torch.cuda.max_memory_allocated() / 2 ** 30)
    return {k: {"ms": statistics.median(v), "peak_gib": peak[k]} for k, v in times.items()}


# ---- one (336, 256) layer on the batch's 9-neighbour graph
ptr32 = batch.ptr.to(torch.int32)
gr = ops.knn_graph(batch.x, [0, 1, 2], batch.batch.to(torch.int32), ptr32, K, plan=ops.knn_plan(ptr32, N))
cr = ops.compact_rows(gr)
cr.reverse_view()
PQ = torch.randn(N, 2 * H1p, device="cuda")
W2, b2 = torch.randn(H2, H1, device="cuda") / H1 ** 0.5, torch.zeros(H2, device="cuda")
ln1 = (torch.ones(H1, device="cuda"), torch.zeros(H1, device="cuda"))
ln2 = (torch.ones(H2, device="cuda"), torch.zeros(H2, device="cuda"))
gout = torch.randn(N, H2, device="cuda")
W2p, W2Tp, W2g, W2Tg = (ops.pack_weight(W2, [H1], dt, 32), ops.pack_weight(W2.t(), [H2], dt, 32),
                        ops.pack_weight(W2, [H1], dt, ops.gemm_kunit(mode)), ops.pack_weight(W2.t(), [H2], dt, ops.gemm_kunit(mode)))
lowp, r16 = ("only" if mode == ops.MODE_BF16 else "no"), mode == ops.MODE_BF16


def fused_layer(bwd):
    out, st = ops.edgeconv_norm_fwd(mode, cr, PQ, H1p, H1, H2, W2p, b2, ln1, ln2)
    if bwd:
        dPQ = torch.empty((N, 2 * H1p), dtype=dt, device="cuda")
        a1, dz2, dpre1, *_ = ops.edgeconv_norm_bwd(mode, cr, PQ, H1p, H1, H2, W2p, W2Tp, b2, ln1, ln2, st, gout, dPQ[:, :H1p])
        ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
        ops.edgeconv_dq_gather(mode, cr.reverse_view(), dpre1, H1p, dPQ[:, H1p:])


def unfused_layer(bwd):
    pre1 = ops.edge_gather_pre(PQ, H1p, cr.ic, cr.jc, lowp=r16)
    a1, st1 = ops.rownorm_act_fwd(pre1, H1, "gelu", *ln1, valid=cr.jc, cpad=H1p, lowp=lowp)
    z2 = ops.linear_fwd(mode, [(a1, H1p)], W2g, H2, bias=b2, out_cols=H2, out_lowp=r16)
    m, st2 = ops.rownorm_act_fwd(z2, H2, "gelu", *ln2, valid=cr.jc, cpad=H2, lowp=lowp)
    cr.sum(m, H2)
    if bwd:
        dz2, _, _ = ops.rownorm_act_bwd(gout, z2, H2, "gelu", *ln2, st2, valid=cr.jc, gidx=cr.ic, cpad=H2, lowp=lowp)
        ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
        da1 = ops.linear_fwd(mode, [(dz2, H2)], W2Tg, H1, out_cols=H1p, out_lowp=r16)
        dpre1, _, _ = ops.rownorm_act_bwd(da1, pre1, H1, "gelu", *ln1, st1, valid=cr.jc, cpad=H1p, lowp=lowp)
        dPQ = torch.empty((N, 2 * H1p), dtype=dt, device="cuda")
        dPQ[:, :H1p] = cr.sum(dpre1, H1p)
        ops.edgeconv_dq_gather(mode, cr.reverse_view(), dpre1, H1p, dPQ[:, H1p:])


res = {"layer_fwd": alternate({"unfused": lambda: unfused_layer(False), "fused": lambda: fused_layer(False)}),
       "layer_fwd_bwd": alternate({"unfused": lambda: unfused_layer(True), "fused": lambda: fused_layer(True)})}
print(json.dumps({"layer": res}), flush=True)

# ---- the four-layer DynEdge DeepIce embeds, one training step
model = g.DynEdge(9, nb_neighbours=9, post_processing_layer_sizes=[336, 384], dynedge_layer_sizes=[(128, 256), (336, 256), (336, 256), (336, 256)],
                  global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True).to("cuda")
opt = torch.optim.AdamW(model.parameters(), lr=1e-5, fused=True)


def step(fused):
    model.set_backend(dtype=dtype, fused_norm_edge=fused)
    opt.zero_grad(set_to_none=True)
    (model(batch).float() ** 2).mean().backward()
    opt.step()


res["dynedge_step"] = alternate({"unfused": lambda: step(False), "fused": lambda: step(True)})
print(json.dumps({"metric": "ms per call, LayerNorm + GELU edge MLP fused vs unfused", "B": B, "pulses": N, "k": K, "dtype": dtype,
                  "reps_per_window": reps, "windows": 5, **res}))
