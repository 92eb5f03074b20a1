#!/usr/bin/env python3
"""gn_icemix_nodes (IceMixNodes: models/graphs/nodes/nodes.py:309-453) on synthetic IceCube-86 events with the columns
x, y, z, time, charge, auxiliary in the IceCubeKaggle standardisation, ice columns on: the whole call (with its read-back of
the node count) and the two kernels alone (the C entry on preallocated buffers) by device events, at max_pulses = 768, where
almost every event is a copy, and at 192; beside them the same class's host path on the same events (host clock) and
gn_dom_time_series on the same batch.

The ice table is read from $GRAPHNET_AMD_ICE_TABLE, by default the fixture of the test suite.

usage: run_icemix_nodes.py [B]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GRAPHNET_AMD_ICE_TABLE", os.path.join(ROOT, "tests", "golden", "ice_transparency.npz"))
import graphnet_amd as g                                              # noqa: E402
from graphnet_amd import _lib, ops                                    # noqa: E402
from graphnet_amd.synthetic import synthetic_icecube86_raw            # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
NAMES = ["x", "y", "z", "time", "charge", "auxiliary"]
torch.manual_seed(0)
raw, ptr, _ = synthetic_icecube86_raw(B, seed=5)
x = torch.from_numpy(raw[:, :6].copy())
x[:, 5] = (torch.rand(x.shape[0]) < 0.3).float()                      # auxiliary flag
x = g.IceCubeKaggle()(x.to("cuda"), NAMES)
ptr32 = torch.from_numpy(ptr).to(torch.int32).to("cuda")
n = np.diff(ptr)
N = int(x.shape[0])


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


results = {}
for L in (768, 192):
    nd = g.IceMixNodes(input_feature_names=NAMES, max_pulses=L, z_name="z", hlc_name="auxiliary")
    nodes, node_ptr, ids = nd.sample_batch(x, ptr32, seed=1)
    table = nd._table(x.device)
    out = torch.empty((N, 8), dtype=torch.float32, device="cuda")
    optr = torch.empty(B + 1, dtype=torch.int32, device="cuda")
    oids = torch.empty(N, dtype=torch.int32, device="cuda")
    lib = _lib.lib()

    def kernels():
        _lib.check(lib.gn_icemix_nodes(x.data_ptr(), x.stride(0), 6, N, ptr32.data_ptr(), B, L, 5, 2, table.data_ptr(),
                                       int(table.shape[1]), 1, None, 32, out.data_ptr(), 8, optr.data_ptr(), oids.data_ptr(),
                                       ops._st()))

    ms_call = timed(lambda: nd.sample_batch(x, ptr32, seed=1))         # includes the read-back of M
    ms_kernels = timed(kernels)
    assert torch.equal(out[:len(nodes)], nodes) and torch.equal(oids[:len(ids)], ids)
    xc, pc = x.cpu(), ptr32.cpu()
    nd.sample_batch(xc, pc, seed=1)
    t0 = time.perf_counter()
    for _ in range(3):
        host = nd.sample_batch(xc, pc, seed=1)
    ms_host = 1e3 * (time.perf_counter() - t0) / 3
    assert torch.equal(host[2], ids.cpu()) and torch.equal(host[0].view(torch.int32), nodes.cpu().view(torch.int32))
    traffic = int(nodes.shape[0]) * (6 + 8 + 1) * 4 + (B + 1) * 8      # the kept rows of x read; rows, ids and node_ptr written
    results[L] = {"ms_call": ms_call, "ms_kernels": ms_kernels, "ms_host_path": ms_host, "nodes": int(nodes.shape[0]),
                  "events_cut": int((n > L).sum()), "traffic_mb": traffic / 1e6}
    print(f"B={B} pulses={N} max_pulses={L}: {int((n > L).sum())} events cut, {int(nodes.shape[0])} nodes; call {ms_call:.3f} ms  "
          f"kernels {ms_kernels:.3f} ms  host path {ms_host:.1f} ms", flush=True)

dts = g.NodeAsDOMTimeSeries()
pulses = x[:, :5].contiguous()
ms_dts = timed(lambda: dts.series_batch(pulses, ptr32))
print(f"gn_dom_time_series on the same batch: {ms_dts:.3f} ms", flush=True)
print(json.dumps({"metric": "ms per gn_icemix_nodes call, synthetic IceCube-86", "events": B, "pulses": N,
                  "longest_event": int(n.max()), "gn_dom_time_series_ms": ms_dts,
                  "max_pulses": {str(k): v for k, v in results.items()}}))
