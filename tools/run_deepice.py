#!/usr/bin/env python3
"""DeepIce (models/gnn/icemix.py) in the shape of the pretrained B_d32 configuration (hidden_dim 768, head_size 32, 12 blocks
after 4 sandwich blocks) on synthetic IceCube-86 events capped at 192 pulses (x, y, z, time, charge, auxiliary in the
IceCubeKaggle standardisation): fwd + bwd + AdamW per step of the backbone alone (a mean-square dummy loss on its latent), for
n_rel = 1 (the shipped value) and n_rel = 4.  The biased attention (gn_rel_attention_fwd / _bwd) is also timed on its own with
device events, beside the plain ragged attention (fp32 and bf16 kernels) on the same batch and the same qkv.

--icemix builds the batch as a user of the reference does, through IceMixNodes(max_pulses=192) on the device (one
gn_icemix_nodes call: a random 192 of each longer event, the auxiliary flag flipped) in place of the host loop that keeps the
first 192; the default workload is the host loop, so that its numbers stay comparable with earlier ones.

usage: run_deepice.py [B] [fp32|bf16] [steps] [--icemix]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphnet_amd as g                                              # noqa: E402
from graphnet_amd import ops                                          # noqa: E402
from graphnet_amd.synthetic import synthetic_icecube86_raw            # noqa: E402

ICEMIX = "--icemix" in sys.argv
argv = [a for a in sys.argv if a != "--icemix"]
B = int(argv[1]) if len(argv) > 1 else 1024
dtype = argv[2] if len(argv) > 2 else "bf16"
steps = int(argv[3]) if len(argv) > 3 else 10
MAX_PULSES, HIDDEN, HEAD = 192, 768, 32
torch.manual_seed(0)

NAMES = ["x", "y", "z", "time", "charge", "auxiliary"]
raw, ptr, _ = synthetic_icecube86_raw(B, seed=5)
if ICEMIX:
    raw = raw[:, :6].copy()
    raw[:, 5] = (torch.rand(raw.shape[0]) < 0.3).float().numpy()     # auxiliary flag
    nodes = g.IceMixNodes(input_feature_names=NAMES, max_pulses=MAX_PULSES, z_name="z", hlc_name="auxiliary",
                          add_ice_properties=False)                  # DeepIce reads the first six columns
    batch = g.KNNGraph(g.IceCubeKaggle(), node_definition=nodes, input_feature_names=NAMES).batch_from_raw(
        [raw[ptr[i]:ptr[i + 1]] for i in range(B)], NAMES, device="cuda")
    n = (batch.ptr[1:] - batch.ptr[:-1]).cpu().numpy()
    B = len(n)                                                        # events of one pulse are dropped
    x = batch.x
else:
    keep = np.concatenate([np.arange(ptr[i], min(ptr[i + 1], ptr[i] + MAX_PULSES)) for i in range(B)])      # the first 192 pulses
    n = np.minimum(ptr[1:] - ptr[:-1], MAX_PULSES)
    x = torch.from_numpy(raw[keep][:, :6].copy())
    x[:, 5] = (torch.rand(x.shape[0]) < 0.3).float()                      # auxiliary flag
    x = g.IceCubeKaggle()(x, NAMES)
    ptr_t = torch.from_numpy(np.concatenate([[0], np.cumsum(n)])).to(torch.int64)
    batch = g.Batch(x=x.to("cuda"))
    batch.ptr = ptr_t.to("cuda")
    batch.batch = torch.repeat_interleave(torch.arange(B), torch.from_numpy(n)).to("cuda")
    batch.n_pulses = torch.from_numpy(n).to(torch.int32).to("cuda")
N = int(x.shape[0])
pairs = int((n.astype(np.int64) ** 2).sum())


def timed(fn, reps=10, warm=2):
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


# the attention kernels alone, one layer of the B_d32 shape (24 heads of 32)
H = HIDDEN // HEAD
ptr32 = batch.ptr.to(torch.int32)
plan = ops.attention_plan(ptr32)
qkv = torch.randn(N, 3 * HIDDEN, device="cuda")
qp = torch.randn(N, HIDDEN, device="cuda") * 0.5
xt = batch.x[:, :4].contiguous()
freq = ops.rel_attention_freq(HEAD, "cuda")
out, u, lse2 = ops.rel_attention_fwd(qkv, qp, xt, freq, H, ptr32, plan)
dout, du = torch.randn_like(out), torch.randn_like(u)
pieces = {
    "rel_attention_fwd": timed(lambda: ops.rel_attention_fwd(qkv, qp, xt, freq, H, ptr32, plan)),
    "rel_attention_bwd": timed(lambda: ops.rel_attention_bwd(qkv, qp, xt, freq, H, ptr32, plan, out, u, lse2, dout, du)),
}
o32, l32 = ops.attention_fwd(qkv, H, ptr32, plan)
pieces["attention_fwd_fp32"] = timed(lambda: ops.attention_fwd(qkv, H, ptr32, plan))
pieces["attention_bwd_fp32"] = timed(lambda: ops.attention_bwd(qkv, H, ptr32, plan, o32, l32, dout))
qkv16, dout16 = qkv.to(torch.bfloat16), dout.to(torch.bfloat16)
o16, l16 = ops.attention_fwd(qkv16, H, ptr32, plan)
pieces["attention_fwd_bf16"] = timed(lambda: ops.attention_fwd(qkv16, H, ptr32, plan))
pieces["attention_bwd_bf16"] = timed(lambda: ops.attention_bwd(qkv16, H, ptr32, plan, o16, l16, dout16))
print(f"B={B} pulses={N} pairs={pairs} heads={H}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in pieces.items()), flush=True)
del qkv, qp, out, u, dout, du, o32, o16, qkv16, dout16

results = {}
for n_rel in (1, 4):
    m = g.DeepIce(hidden_dim=HIDDEN, head_size=HEAD, depth=12, depth_rel=4, n_rel=n_rel, seq_length=192).to("cuda")
    m.set_backend(dtype=dtype)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-5, eps=1e-7, weight_decay=0.05, fused=True)

    def step():
        opt.zero_grad(set_to_none=True)
        y = m(batch)
        loss = (y.float() ** 2).mean()
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        l = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        l = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    ops.enable_timers(True)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    summary = ops.timer_summary()
    ops.enable_timers(False)
    results[n_rel] = {"ms_per_step": 1e3 * dt, "events_per_s": B / dt, "loss": float(l),
                      "phase_ms_per_step": {k: ms / 3 for k, (n_, ms) in sorted(summary.items(), key=lambda kv: -kv[1][1])}}
    print(f"DeepIce B_d32 n_rel={n_rel} B={B} {dtype}: {1e3 * dt:.2f} ms/step  {B / dt:.0f} events/s  loss {float(l):.4f}", flush=True)
    del m, opt

peak = torch.cuda.max_memory_allocated() / 2**30
print(json.dumps({
    "metric": "events/sec DeepIce (B_d32 shape: hidden 768, 24 heads of 32, 4 + 12 blocks, n_rel 1) fwd+bwd+AdamW, synthetic IceCube-86",
    "value": results[1]["events_per_s"], "unit": "events/s", "n_gpus": 1, "steps": steps, "ms_per_step": results[1]["ms_per_step"],
    "ms_per_step_n_rel4": results[4]["ms_per_step"], "dtype": dtype, "data": "synthetic",
    "config": {"workload": "DeepIce(hidden_dim=768, head_size=32, depth=12, depth_rel=4, seq_length=192) on synthetic IceCube-86 "
                           "events capped at 192 pulses", "events_per_gpu": B, "pulses_per_gpu": N, "pairs_per_gpu": pairs},
    "pieces_ms": pieces,
    "rel_over_plain_fp32": (pieces["rel_attention_fwd"] + pieces["rel_attention_bwd"]) /
                           (pieces["attention_fwd_fp32"] + pieces["attention_bwd_fp32"]),
    "peak_mem_gib": peak,
    "phase_ms_per_step": {str(k): v["phase_ms_per_step"] for k, v in results.items()}}))
