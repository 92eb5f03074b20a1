#!/usr/bin/env python3
"""RNN_TITO (models/gnn/RNN_tito.py: Node_RNN + DynEdgeTITO; GRU hidden size 64, two layers of which layer 0 reaches the
output, four DynTrans layers 256/256, 16 heads, 8 neighbours on x, y, z, t) on the bench.py workload: synthetic IceCube-86
pulses (x, y, z, time, charge) regrouped into DOM time series by NodeAsDOMTimeSeries; fwd + bwd + Adam per step of the
backbone alone (a mean-square dummy loss on its latent).  The pieces are also timed on their own with device events:
gn_dom_time_series and the GRU forward and backward entries before the steps, and after them torch.nn.GRU (rocm's own
kernels) over the same series packed with pack_sequence, which is what the reference runs.

usage: run_rnn_tito.py [B] [fp32|bf16] [steps]"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphnet_amd as g                                              # noqa: E402
from graphnet_amd import ops                                          # noqa: E402
from graphnet_amd.synthetic import synthetic_icecube86_batch          # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
dtype = sys.argv[2] if len(sys.argv) > 2 else "bf16"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
torch.manual_seed(0)
src = synthetic_icecube86_batch(B, seed=5).to("cuda")
pulses = src.x[:, :5].contiguous()                                     # dom_x, dom_y, dom_z, dom_time, charge
ptr32 = src.ptr.to(torch.int32)
nd = g.NodeAsDOMTimeSeries()


def timed(fn, reps=20, warm=3):
    """ms per call by device events."""
    for _ in range(warm):
        fn()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / reps


rows, series_ptr, dom_ptr = nd.series_batch(pulses, ptr32)
N, M = int(rows.shape[0]), int(series_ptr.shape[0]) - 1
ms_nodes = timed(lambda: nd.series_batch(pulses, ptr32))               # includes the read-back of M

m = g.RNN_TITO(5, [4, 3], features_subset=[0, 1, 2, 3]).to("cuda")
m.set_backend(dtype=dtype)
gru = m._rnn._rnn
xs = rows[:, [4, 3]].contiguous()
w = [gru.weight_ih_l0.detach(), gru.weight_hh_l0.detach(), gru.bias_ih_l0.detach(), gru.bias_hh_l0.detach()]
out, saved = ops.gru_series_fwd(xs, series_ptr, *w)
dout = torch.randn_like(out)
ms_gru_fwd = timed(lambda: ops.gru_series_fwd(xs, series_ptr, *w))
ms_gru_bwd = timed(lambda: ops.gru_series_bwd(dout, saved, xs, series_ptr, w[1]))

sp = series_ptr.cpu()
lengths = (sp[1:] - sp[:-1]).to(torch.int64)
print(f"B={B} pulses={N} series={M} longest={int(lengths.max())}: gn_dom_time_series {ms_nodes:.3f} ms   GRU fwd {ms_gru_fwd:.3f} ms   "
      f"GRU bwd {ms_gru_bwd:.3f} ms", flush=True)

b = g.Batch(x=rows, ptr=src.ptr, batch=src.batch, n_pulses=src.n_pulses)
b.series_ptr, b.dom_ptr = series_ptr, dom_ptr
opt = torch.optim.Adam(m.parameters(), lr=1e-4, eps=1e-3, fused=True)


def step():
    opt.zero_grad(set_to_none=True)
    y = m(b)
    loss = (y.float() ** 2).mean()
    loss.backward()
    opt.step()
    return loss


for _ in range(10):
    l = step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    l = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
ops.enable_timers(True)
for _ in range(steps):
    step()
torch.cuda.synchronize()
summary = ops.timer_summary()
ops.enable_timers(False)
peak = torch.cuda.max_memory_allocated() / 2**30
print(f"RNN_TITO B={B} {dtype}: {1e3*dt:.2f} ms/step  {B/dt:.0f} events/s  loss {float(l):.4f}  peak mem {peak:.2f} GiB", flush=True)

# what the kernel replaces: torch.nn.GRU over the packed series (the split and the packing are not in the timed part)
packed = torch.nn.utils.rnn.pack_sequence(list(xs.split(lengths.tolist())), enforce_sorted=False)
ref_gru = torch.nn.GRU(input_size=2, hidden_size=64, num_layers=1, batch_first=True).to("cuda")


def torch_gru_step():
    ref_gru.zero_grad(set_to_none=True)
    (ref_gru(packed)[-1][0] * dout).sum().backward()


ms_torch_fwd = timed(lambda: ref_gru(packed)[-1][0], reps=5, warm=2)
ms_torch_fwd_bwd = timed(torch_gru_step, reps=5, warm=2)
print(f"  torch.nn.GRU on the packed series: fwd {ms_torch_fwd:.2f} ms, fwd+bwd {ms_torch_fwd_bwd:.2f} ms", flush=True)
print(json.dumps({
    "metric": "events/sec RNN_TITO (Node_RNN GRU 64 + DynEdgeTITO 4 x 256/256, 16 heads) fwd+bwd+Adam, synthetic IceCube-86",
    "value": B / dt, "unit": "events/s", "n_gpus": 1, "steps": steps, "ms_per_step": 1e3 * dt, "dtype": dtype, "data": "synthetic",
    "config": {"workload": "RNN_TITO(5, [4, 3], features_subset=[0, 1, 2, 3]) on NodeAsDOMTimeSeries rows of synthetic IceCube-86 "
                           "pulses", "events_per_gpu": B, "pulses_per_gpu": N, "series_per_gpu": M,
               "longest_series": int(lengths.max())},
    "pieces_ms": {"gn_dom_time_series": ms_nodes, "gru_series_fwd": ms_gru_fwd, "gru_series_bwd": ms_gru_bwd,
                  "torch_nn_gru_packed_fwd": ms_torch_fwd, "torch_nn_gru_packed_fwd_bwd": ms_torch_fwd_bwd},
    "peak_mem_gib": peak,
    "phase_ms_per_step": {k: ms / steps for k, (n_, ms) in sorted(summary.items(), key=lambda kv: -kv[1][1])}}))
