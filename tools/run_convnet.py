#!/usr/bin/env python3
"""ConvNet (reference models/gnn/convnet.py: three TAGConv(K=2) layers, add|max pooling, BatchNorm1d, five Linear layers) +
energy head under StandardModel on the bench.py workload (synthetic IceCube-86 pulses, k = 8 graph built once on the device):
fwd + bwd + Adam per step.  The TAGConv kernels are also timed one by one with device events on the width-128 layer of the same
batch (gn_tag_propagate, gn_tag_propagate_t, gn_tagconv_fwd), beside the same layer composed from torch device ops
(index_select / index_add_ with the edge weights, then three Linears + leaky ReLU; its forward alone and forward + backward).

usage: run_convnet.py [B] [fp32|bf16] [steps] [--warm N] [--reps N]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphnet_amd as g                                              # noqa: E402
from graphnet_amd import ops                                          # noqa: E402
from graphnet_amd.synthetic import synthetic_icecube86_batch          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=1024)
ap.add_argument("dtype", nargs="?", default="bf16", choices=["bf16", "fp32"])
ap.add_argument("steps", nargs="?", type=int, default=20)
ap.add_argument("--warm", type=int, default=10, help="calls / optimizer steps before the timed ones")
ap.add_argument("--reps", type=int, default=50, help="timed calls per kernel; repeated 5 times for the spread")
cli = ap.parse_args()
B, dtype, steps = cli.B, cli.dtype, cli.steps
mode = {"fp32": ops.MODE_F32, "bf16": ops.MODE_BF16}[dtype]
torch.manual_seed(0)
b = synthetic_icecube86_batch(B, seed=5).to("cuda")
N, C, K = int(b.x.shape[0]), 128, 8
ptr32 = b.ptr.to(torch.int32)
table = ops.knn_graph(b.x.float(), [0, 1, 2], b.batch.to(torch.int32), ptr32, K)
b.nbr_table = table                                                   # the loader's static graph, already a table


def timed(fn):
    """(median, min, max) ms per call over 5 windows of --reps calls, device events."""
    for _ in range(cli.warm):
        fn()
    out = []
    for _ in range(5):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(cli.reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(z) / cli.reps)
    out.sort()
    return out[2], out[0], out[-1]


# ---- the kernels of one width-128 layer
dis = ops.tag_norm(table)
table.build_reverse()
x = torch.randn(N, C, device="cuda")
conv = g.TAGConv(C, C).to("cuda")
Wp = ops.tagconv_pack([l.weight for l in conv.lins], mode)
h1 = ops.tag_propagate(x, C, table, dis)
pieces = {
    "tag_propagate": timed(lambda: ops.tag_propagate(x, C, table, dis, out=h1)),
    "tag_propagate_t": timed(lambda: ops.tag_propagate_t(x, C, table, dis, add=h1)),
    "tagconv_fwd": timed(lambda: ops.tagconv_fwd(mode, x, h1, table, dis, Wp, conv.bias.detach(), C, C)),
}
xg = x.clone().requires_grad_()
gout = torch.randn(N, C, device="cuda")


def layer_fb(fwd, inp):
    inp.grad = None
    fwd(inp).backward(gout)


pieces["layer_fwd"] = timed(lambda: conv(x, table, dis, mode))
pieces["layer_fwd_bwd"] = timed(lambda: layer_fb(lambda t: conv(t, table, dis, mode), xg))

# ---- the comparator: the same layer from torch device ops on the same edges
ei = table.edge_index()
src, dst = ei[0], ei[1]
w = (dis[src] * dis[dst]).unsqueeze(1)
lins = [l.weight.detach().clone().requires_grad_() for l in conv.lins]
bias = conv.bias.detach().clone().requires_grad_()


def torch_layer(t):
    out, h = torch.nn.functional.linear(t, lins[0], bias), t
    for W in lins[1:]:
        h = torch.zeros_like(h).index_add_(0, dst, h.index_select(0, src) * w)
        out = out + torch.nn.functional.linear(h, W)
    return torch.nn.functional.leaky_relu(out, 0.01)


with torch.no_grad():
    pieces["torch_layer_fwd"] = timed(lambda: torch_layer(x))
pieces["torch_layer_fwd_bwd"] = timed(lambda: layer_fb(torch_layer, xg))
print(f"B={B} pulses={N} edges={int(ei.shape[1])} {dtype}: " + "  ".join(f"{k} {v[0]:.3f} ms" for k, v in pieces.items()), flush=True)

# ---- the whole model
m = g.StandardModel(
    graph_definition=g.KNNGraph(g.IceCube86(), nb_nearest_neighbours=8),
    backbone=g.ConvNet(7, 128),
    tasks=[g.EnergyReconstruction(hidden_size=128, loss_function=g.LogCoshLoss(),
                                  transform_prediction_and_target=torch.log10)],
    optimizer_kwargs={"lr": 1e-4, "eps": 1e-3}).to("cuda")
m.backbone.set_backend(dtype=dtype)
opt = torch.optim.Adam(m.parameters(), lr=1e-4, eps=1e-3, fused=True)


def step():
    opt.zero_grad(set_to_none=True)
    loss = m.shared_step(b)
    loss.backward()
    opt.step()
    return loss


for _ in range(cli.warm):
    l = step()
torch.cuda.synchronize()
times = []
for _ in range(steps):
    t0 = time.perf_counter()
    l = step()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
times.sort()
dt = times[len(times) // 2]
print(json.dumps({
    "metric": "events/sec ConvNet(7, 128) + energy head fwd+bwd+Adam, synthetic IceCube-86, k = 8",
    "value": B / dt, "unit": "events/s", "n_gpus": 1, "steps": steps, "ms_per_step": 1e3 * dt,
    "ms_per_step_min_max": [1e3 * times[0], 1e3 * times[-1]], "dtype": dtype, "data": "synthetic", "loss": float(l),
    "config": {"events_per_gpu": B, "pulses_per_gpu": N, "edges": int(ei.shape[1]), "warm": cli.warm, "reps": cli.reps},
    "pieces_ms_median_min_max": {k: [round(t, 4) for t in v] for k, v in pieces.items()},
    "peak_mem_gib": torch.cuda.max_memory_allocated() / 2**30}))
