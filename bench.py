#!/usr/bin/env python3
"""bench.py — events/s for DynEdge fwd+bwd(+Adam, +gradient all-reduce) on synthetic IceCube-86
pulse graphs (BASELINE.json metric; workload = configs[1] at N = 1, configs[2] at N > 1),
one process per GPU.

    python bench.py --gpus N --steps K --warmup W                  # starts the N ranks itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Launching (the reference gets this from Lightning: ``Trainer(strategy="ddp", devices=gpus)``,
``models/easy_model.py:83-112``): when ``--gpus N > 1`` and ``WORLD_SIZE`` is not set, this process is only a
launcher.  It makes NO ``torch.cuda`` / HIP call at all (not even a device count; never ``exec``) and starts N children of itself with
``RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT``, forwards rank 0's single JSON line
and exits non-zero if any child fails.  Under ``torch.distributed.run`` the environment is already there and
``--gpus`` must equal ``WORLD_SIZE`` (otherwise the run would silently measure something else: exit 2).

A step = one pass of the hot path over one batch of B events already resident in HBM:
layer-1 k-NN build, global variables, 4x(P|Q GEMM, fused EdgeConv, re-kNN), post MLP, pooling,
readout, energy head, LogCosh, full backward, one flat RCCL all-reduce (N > 1), Adam step.
Rank 0 prints ONE JSON line.

A plain run does what the headline figure needs and nothing else: set-up, ramp-up, W warm-up steps, the K timed
steps, the result line (``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` = the
milliseconds one timed step took, and the facts of the timed region itself).  ``--full`` adds every other measurement
and check to the same line: clock samples and graph ties of the timed region, the config-3 facts (replica equality,
all-reduce cost), per-op HIP-event timers with `roofline` / `path_roofline`, a second batch size, the fp32 mode, the
library yardsticks and `cpu_baseline` with the in-run parity gate (exit code 3 when it fails).

``--dump-outputs DIR`` writes what the LAST timed step handed to its caller as ``DIR/<name>.npy`` (float32):
``prediction`` (the task output per event), ``loss``, ``grad`` (the flat gradient after the all-reduce) and ``weights``
(every parameter after the optimizer step, flattened in ``parameters()`` order).  Inputs and initial weights are
seeded and the number of steps before the timed region is fixed in such a run, so two builds compare array for array.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3
RAMP_UP_STEPS = 80             # untimed steps before the W warm-up steps, at least (clock / allocator ramp: ramp_up())
RAMP_UP_MAX_S = float(os.environ.get("GN_BENCH_RAMP_MAX_S", "20"))   # ... and at most this long while the step time still moves
RAMP_UP_MAX_S_PLAIN = 10.0     # ... in a plain run (no --full), whose time outside the steps is part of its cost
DUMP_MAX_BYTES = 64 << 20      # --dump-outputs: all arrays together
TRAFFIC_FILE = os.path.join("profiles", os.environ.get("GN_TRAFFIC_FILE", "r03_traffic.json"))


# ------------------------------------------------------------------------------------------- launcher
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, argv, dry: bool) -> int:
    """Parent of an N-rank run: one child per rank, rank 0's stdout forwarded, non-zero if any rank fails.
    Nothing here touches the GPU or loads HIP: the parent does not even count devices (every child refuses with
    exit code 2 when it sees fewer GPUs than ranks, and that code is propagated).  Rank 0's stdout is drained by a
    reader thread while the ranks run (its JSON line plus library chatter can exceed a pipe buffer, and a rank
    blocked in ``write`` would leave the others waiting in the final barrier); an overall wall-clock limit
    (``GN_BENCH_LAUNCH_TIMEOUT`` seconds, default 1500) ends a run that hangs."""
    import threading
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr))
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.monotonic() + float(os.environ.get("GN_BENCH_LAUNCH_TIMEOUT", "1500"))
    rc = 0
    pending = set(range(n))
    while pending:
        for r in sorted(pending):
            code = procs[r].poll()
            if code is None:
                continue
            pending.discard(r)
            rc = rc or code
        if pending and time.monotonic() > deadline:
            print("[bench] launcher time limit reached: terminating the ranks", file=sys.stderr)
            rc = rc or 124
        if rc != 0:                      # one rank died: the others would wait in a collective for ever
            for r in pending:
                procs[r].terminate()
            for r in pending:
                try:
                    procs[r].wait(timeout=20)
                except subprocess.TimeoutExpired:
                    procs[r].kill()
            break
        time.sleep(0.05)
    reader.join(timeout=30)
    out0 = (b"".join(c for c in chunks if c) or b"").decode(errors="replace")
    for line in out0.splitlines():       # the JSON line to stdout; library chatter (gloo prints its peers) to stderr
        print(line, file=sys.stdout if line.lstrip().startswith("{") else sys.stderr)
    sys.stdout.flush()
    if rc != 0:
        print(f"[bench] a rank exited with code {rc}", file=sys.stderr)
    return rc


# ------------------------------------------------------------------------------------------- config-3 facts
def weights_checksum(module: torch.nn.Module) -> torch.Tensor:
    """Two int64 words over the BITS of every parameter (order-sensitive): equal words <=> bitwise equal weights."""
    flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in module.parameters()])
    bits = flat.view(torch.int32).to(torch.int64)
    idx = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
    return torch.stack([bits.sum(), (bits * idx).sum()])


def weights_identical_across_ranks(module: torch.nn.Module) -> bool:
    cs = weights_checksum(module)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return True
    box = [torch.empty_like(cs) for _ in range(dist.get_world_size())]
    dist.all_gather(box, cs)
    return all(torch.equal(b, box[0]) for b in box)


def allreduce_us(sync, reps: int = 20) -> float:
    """Latency of the step's ONE exchange: the flat-gradient all-reduce alone, back to back, in microseconds."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return 0.0
    cuda = sync.flat.is_cuda
    saved = sync.flat.clone()
    for _ in range(3):
        sync.all_reduce()
    if cuda:
        torch.cuda.synchronize()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        sync.all_reduce()
    if cuda:
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sync.flat.copy_(saved)
    t = torch.tensor([dt], dtype=torch.float64, device=sync.flat.device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return 1e6 * float(t.item()) / reps


def run_dry(args, rank: int, world: int) -> None:
    """``--dry-run``: the launcher, rendezvous, flat all-reduce and the config-3 report fields on CPU over gloo with a
    stand-in network - no kernel runs and ``value`` is null.  For the CPU test of the N-rank control flow only."""
    from graphnet_amd.parallel import FlatGradAllReduce, broadcast_parameters
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)                        # different initial weights per rank ...
    net = torch.nn.Sequential(torch.nn.Linear(7, 32), torch.nn.ReLU(), torch.nn.Linear(32, 1))
    broadcast_parameters(net)                            # ... made identical, as in the real run
    sync = FlatGradAllReduce(net.parameters())
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-3)
    gen = torch.Generator().manual_seed(20241016 + rank)
    x = torch.randn(64, 7, generator=gen)
    t0 = time.perf_counter()
    for _ in range(args.warmup + args.steps):
        sync.zero_grad()
        net(x).pow(2).mean().backward()
        sync()
        opt.step()
    dt = time.perf_counter() - t0
    same = weights_identical_across_ranks(net)
    us = allreduce_us(sync, reps=5)
    if rank == 0:
        print(json.dumps({"metric": "events/sec DynEdge fwd+bwd, IceCube-86 k=8", "value": None, "unit": "events/s",
                          "n_gpus": dist.get_world_size() if world > 1 else 1, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": 1e3 * dt / max(args.steps + args.warmup, 1), "dry_run": True,
                          "backend": dist.get_backend() if world > 1 else None,
                          "allreduce_us_per_step": us, "weights_identical_across_ranks": same}))
        sys.stdout.flush()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------- the workload
def build_model(dtype: str):
    import graphnet_amd as g
    torch.manual_seed(20241016)                       # identical initial weights on every rank
    m = g.StandardModel(
        graph_definition=g.KNNGraph(g.IceCube86()),
        backbone=g.DynEdge(7, global_pooling_schemes=["min", "max", "mean", "sum"]),
        tasks=[g.EnergyReconstruction(hidden_size=128, loss_function=g.LogCoshLoss(),
                                      transform_prediction_and_target=torch.log10)],
        optimizer_kwargs={"lr": 1e-3, "eps": 1e-3},
    )
    m.backbone.set_backend(dtype=dtype)
    return m


def measured_peaks(dev) -> dict:
    """Yardsticks measured in this run: a large library bf16 GEMM (hipBLASLt through
    torch.matmul) and a device-to-device copy.  Not used as denominators: `roofline.peak` stays the
    MI355X_MICROARCH.md figure (2.5 PFLOP/s dense bf16, 8 TB/s HBM)."""
    n = 8192
    a = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
    b = torch.randn(n, n, device=dev, dtype=torch.bfloat16)
    torch.matmul(a, b)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(10):
        torch.matmul(a, b)
    e1.record()
    torch.cuda.synchronize()
    gemm = 10 * 2.0 * n ** 3 / (e0.elapsed_time(e1) * 1e-3) / 1e12
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    copy = 10 * 2.0 * (1 << 30) / (e0.elapsed_time(e1) * 1e-3) / 1e9          # read + write bytes
    return {"library_bf16_gemm_tflops": gemm, "hbm_copy_gbs": copy,
            "note": "8192^3 bf16 torch.matmul; 1 GiB device copy (read+write bytes)"}


def algorithmic_flops(n_nodes: int, n_edges: int, n_events: int, F0: int = 19, n_pool: int = 4) -> float:
    """Reference-formulation forward GEMM FLOPs, MAC = 2 FLOP."""
    return 2.0 * (n_edges * (2 * F0 * 128 + 128 * 256) + 3 * n_edges * (512 * 336 + 336 * 256)
                  + n_nodes * ((F0 + 1024) * 336 + 336 * 256) + n_events * (n_pool * 256 * 128 + 128))


def executed_flops(n_nodes: int, n_edges: int, n_events: int, F0: int = 19, n_pool: int = 4) -> float:
    """GEMM FLOPs the HIP path actually EXECUTES per step (fwd + bwd), MAC = 2 FLOP.  The first edge-MLP layer is
    one per-node GEMM (P | Q), so its cost scales with N, not E: forward = P|Q GEMM + edge
    GEMM per conv layer + post MLP + read-out; backward = dW2 and dh per edge, the P|Q weight gradient, the two
    input-gradient contractions of layers 2-4, post-MLP weight and input gradients (raw-feature columns excluded)."""
    conv = [(F0, 128, 256), (256, 336, 256), (256, 336, 256), (256, 336, 256)]
    N, E = float(n_nodes), float(n_edges)
    fwd = sum(2 * N * f * 2 * h1 + 2 * E * h1 * h2 for f, h1, h2 in conv)
    post = 2 * N * ((F0 + 1024) * 336 + 336 * 256)
    head = 2.0 * n_events * (n_pool * 256 * 128 + 128)
    bwd = sum(2 * 2 * E * h1 * h2 + 2 * N * f * 2 * h1 for f, h1, h2 in conv)           # dW2, dh, dW(P|Q)
    bwd += sum(2 * N * 2 * h1 * f for f, h1, _ in conv[1:])                             # d_in of layers 2-4
    bwd += 2 * post - 2 * N * F0 * 336 + 2 * head                                       # post MLP dW + dX, read-out
    return fwd + post + head + bwd


def _log(msg: str) -> None:
    """Progress on stderr: a GPU box kills a command that writes nothing for minutes."""
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def host_cpu() -> dict:
    """Cores this job may use (affinity mask, capped by the cgroup CPU quota when there is one), cores of the
    machine, CPU model string."""
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = None
    try:                                                  # cgroup v2: "<quota> <period>" or "max <period>"
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(float(q) / float(per) + 0.5))
    except (OSError, ValueError):
        pass
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"cores_available": avail, "cgroup_cpu_quota": quota, "cores_machine": os.cpu_count() or avail,
            "cpu_model": model}


def cpu_baseline(events: int, steps: int, warmup: int, parity_model=None, budget_s: float = 45.0):
    """The oracle (plain-torch restatement of the PyG formulation) timed on ALL host cores this job may use
    (3 warm-up + >= 10 timed steps; the timed loop also stops after ``budget_s`` seconds so that a slow
    or oversubscribed host cannot stall the run - the step count actually timed is reported), and - the oracle acting
    as the checker - the parity numbers of the HIP path on a small batch in the same run."""
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    from oracle import dynedge_oracle as orc
    info = host_cpu()
    usable = min(info["cores_available"], info["cgroup_cpu_quota"] or info["cores_available"])
    cores = max(1, int(os.environ.get("GN_CPU_BASELINE_THREADS", usable)))
    torch.set_num_threads(cores)
    torch.manual_seed(20241016)
    m = orc.StandardModelOracle(7, global_pooling_schemes=["min", "max", "mean", "sum"], literal_distribute=True)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-3)
    b = synthetic_icecube86_batch(events, seed=20241016)

    def step():
        ei = orc.knn_graph(b.x, 8, b.batch, [0, 1, 2])          # loader-side k-NN is part of the path
        loss = m.loss(b.x, ei, b.batch, b.n_pulses, b.energy)
        opt.zero_grad()
        loss.backward()
        opt.step()

    _log(f"cpu baseline: {events} events/step on {cores} threads ({info['cpu_model']})")
    tw = time.perf_counter()
    done_w = 0
    for _ in range(warmup):
        step()
        done_w += 1
        if time.perf_counter() - tw > budget_s / 3:
            break
    t0 = time.perf_counter()
    done = 0
    for _ in range(steps):
        step()
        done += 1
        if time.perf_counter() - t0 > budget_s:
            break
    dt = time.perf_counter() - t0
    _log(f"cpu baseline: {done} timed steps in {dt:.1f} s")
    out = {"value": events * done / dt, "unit": "events/s", "cores": cores, "kind": "port",
           "cores_available": info["cores_available"], "cgroup_cpu_quota": info["cgroup_cpu_quota"],
           "cores_machine": info["cores_machine"], "cpu_model": info["cpu_model"],
           "warmup_steps": done_w, "timed_steps": done,
           "sample": f"{done} fwd+bwd+Adam steps (after {done_w} warm-up) of {events} synthetic IceCube-86 events "
                     f"(fp32, torch CPU, {cores} threads = every core this job may use; PyG is not installed: "
                     f"in-repo restatement of the PyG formulation)"}
    if parity_model is not None:
        _log("parity of the HIP path against the oracle (small batch, fp32 and bf16 mode)")
        out["parity"] = parity_vs_oracle(parity_model, orc)
    return out


def parity_vs_oracle(model, orc, events: int = 16) -> dict:
    """SURVEY.md 8d "parity gate in the same run": a small batch through the HIP path (fp32 mode, then bf16 mode)
    against the oracle on the HIP path's own graphs (teacher forcing), layer-1 k-NN table bit for bit."""
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    dev = next(model.parameters()).device
    b = synthetic_icecube86_batch(events, seed=777)
    ref = orc.StandardModelOracle(7, global_pooling_schemes=["min", "max", "mean", "sum"])
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    saved_mode = model.backbone._compute_mode
    res = {"events": events, "tolerance": {"fp32_rel": 1e-4, "bf16_rel": 2e-2}}
    try:
        for name in ("fp32", "bf16"):
            model.backbone.set_backend(dtype=name)
            b.to(dev)
            with torch.no_grad():
                lat, trace = model.backbone(b, return_trace=True)
                pred = model._tasks[0](lat)
            torch.cuda.synchronize()
            b.to("cpu")
            forced = [t.edge_index().cpu() for t in trace["graphs"]]
            with torch.no_grad():
                lat_o = ref.backbone(b.x, forced[0], b.batch, b.n_pulses, forced_edges=forced)
                pred_o = orc.energy_reconstruction(lat_o, ref._affine)
            if name == "fp32":
                res["knn_layer1_bit_exact"] = bool(torch.equal(forced[0], orc.knn_graph(b.x, 8, b.batch, [0, 1, 2])))
            res[f"{name}_latent_max_rel"] = float((lat.float().cpu() - lat_o).abs().max() / lat_o.abs().max())
            res[f"{name}_latent_fro_rel"] = float((lat.float().cpu() - lat_o).norm() / lat_o.norm())
            res[f"{name}_pred_max_rel"] = float(((pred.float().cpu() - pred_o).abs() / pred_o.abs().clamp_min(1e-6)).max())
    finally:
        model.backbone._compute_mode = saved_mode
    # Gate: what north_star names - bit-exact k-NN, fp32 task outputs (and the latent) within 1e-4 rel; bf16 (SURVEY.md 8d:
    # "report max rel err, gate <= 2e-2") on the task outputs and on the latent in the Frobenius norm.  The latent's
    # MAX-norm error in bf16 mode is reported, not gated: on the weights this run has trained it is the worst of 16 x 1024
    # numbers and moves between 0.8 % and 2.2 % with the training trajectory while the kernels' arithmetic is unchanged
    # (tools/probe/parity_ovf.py: identical weights give identical errors on either overflow-row path)
    res["pass"] = bool(res.get("knn_layer1_bit_exact") and res["fp32_latent_max_rel"] < 1e-4 and res["fp32_pred_max_rel"] < 1e-4
                       and res["bf16_pred_max_rel"] < 2e-2 and res["bf16_latent_fro_rel"] < 2e-2)
    res["gated"] = ["knn_layer1_bit_exact", "fp32_latent_max_rel", "fp32_pred_max_rel", "bf16_pred_max_rel", "bf16_latent_fro_rel"]
    return res


def timed_side_run(model, sync, opt, events, seed, dev, world, fence, ramp, steps) -> dict:
    """``steps`` timed training steps on another batch size / mode, after ``ramp`` untimed ones (same model)."""
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    big = synthetic_icecube86_batch(events, seed=seed).to(dev)

    def one():
        sync.zero_grad()
        loss_b = model.shared_step(big)
        loss_b.backward()
        sync()
        opt.step()
    for i in range(ramp):
        one()
        if i % 10 == 9:
            torch.cuda.synchronize()
    fence()
    tb = time.perf_counter()
    for _ in range(steps):
        one()
    fence()
    t = torch.tensor([time.perf_counter() - tb], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return {"events_per_gpu": events, "pulses_per_gpu": int(big.x.shape[0]), "steps": steps,
            "value": events * world * steps / float(t.item()), "unit": "events/s",
            "ms_per_step": 1e3 * float(t.item()) / steps}


class ClockSampler:
    """Best-effort shader-clock / power samples of THIS rank's GPU read from sysfs by a thread (20 Hz) - evidence for
    whether a slow timed region is a uniformly lower clock or a few stalls.  Never fails the run: without readable
    files ``summary()`` is None."""

    def __init__(self, dev: "torch.device"):
        import glob
        import threading
        self.samples, self._stop, self.source = [], threading.Event(), None
        self._f_clk = self._f_pow = self._f_dpm = None
        try:
            pr = torch.cuda.get_device_properties(dev)
            bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
            base = os.path.join("/sys/bus/pci/devices", bdf)
            hw = sorted(glob.glob(os.path.join(base, "hwmon", "hwmon*")))
            for h in hw:
                for name in ("freq1_input",):
                    if self._f_clk is None and os.path.exists(os.path.join(h, name)):
                        self._f_clk = os.path.join(h, name)
                for name in ("power1_average", "power1_input"):
                    if self._f_pow is None and os.path.exists(os.path.join(h, name)):
                        self._f_pow = os.path.join(h, name)
            if os.path.exists(os.path.join(base, "pp_dpm_sclk")):
                self._f_dpm = os.path.join(base, "pp_dpm_sclk")
            self.source = base
        except Exception:
            pass
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _read(self):
        clk = pw = None
        try:
            if self._f_clk:
                clk = float(open(self._f_clk).read()) / 1e6
            elif self._f_dpm:
                for line in open(self._f_dpm).read().splitlines():
                    if line.rstrip().endswith("*"):
                        clk = float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
            if self._f_pow:
                pw = float(open(self._f_pow).read()) / 1e6
        except Exception:
            pass
        return clk, pw

    def _run(self):
        while not self._stop.is_set():
            self.samples.append(self._read())
            self._stop.wait(0.05)

    def start(self):
        if self._f_clk or self._f_dpm or self._f_pow:
            self._thread.start()
        return self

    def stop(self):
        self._stop.set()
        if self._thread.is_alive():
            self._thread.join(timeout=1.0)

    def summary(self):
        def stat(v):
            v = sorted(x for x in v if x is not None)
            return None if not v else {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
        if not self.samples:
            return None
        return {"samples": len(self.samples), "sclk_mhz": stat([c for c, _ in self.samples]),
                "power_w": stat([p_ for _, p_ in self.samples]), "source": self.source}


def graph_ties(model, batch) -> list:
    """Per DynEdgeConv layer of the model AS IT STANDS: [overflow rows ((k+1)-th neighbours of tied distances), sources with
    more than 64 in-edges, largest in-degree] of the graph the layer runs on (one traced forward, outside every timed
    region)."""
    out = []
    try:
        bb = model.backbone
        with torch.no_grad():
            _, tr = bb(batch, return_trace=True)
        for t in tr["graphs"]:
            t.build_reverse()
            deg = t.rev_ptr[1:] - t.rev_ptr[:-1]
            out.append([int(t.ovf_cnt.item()) if t.ovf_cnt is not None else 0, int((deg > 64).sum().item()), int(deg.max().item())])
    except Exception as e:                                      # evidence only: never fails the run
        out = [f"unavailable: {type(e).__name__}: {e}"]
    return out


def ramp_up(step, world: int, dev, min_steps: int, max_s: float, block: int = 10, tol: float = 0.02) -> dict:
    """Untimed steps until the step time has settled: at least ``min_steps``, then blocks of ``block`` steps (HIP events
    around each block, one synchronisation per block) until two consecutive blocks agree with their predecessor within
    ``tol`` or ``max_s`` seconds have passed.  Why: on a cold lease the first seconds of sustained load run slower
    (clock / power-state ramp, allocator growth), and a fixed 80 steps = 2 s at B = 4096 did not always cover it (round 2:
    28.2 ms/step in the driver's run against 22.3 ms of kernel time in the same process a few seconds later).  Every
    step contains the gradient all-reduce, so all ranks must run the same count: the decision is reduced over ranks."""
    t_start = time.perf_counter()
    blocks, done, good = [], 0, 0
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(block):
            step()
        e1.record()
        torch.cuda.synchronize()
        done += block
        blocks.append(e0.elapsed_time(e1) / block)
        if len(blocks) >= 2 and abs(blocks[-1] - blocks[-2]) <= tol * blocks[-2]:
            good += 1
        else:
            good = 0
        more = 1.0 if (done < min_steps or (good < 2 and time.perf_counter() - t_start < max_s)) else 0.0
        if world > 1:
            flag = torch.tensor([more], dtype=torch.float32, device=dev)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            more = float(flag.item())
        if not more:
            break
    return {"steps": done, "seconds": time.perf_counter() - t_start, "settled": good >= 2,
            "block_ms_per_step": [round(b, 3) for b in blocks]}


def kernel_source_hash() -> str:
    """sha256 over the HIP sources and headers of the library: ties a committed PMC measurement to the kernels it
    was taken on (the GPU box has no .git to ask)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "graphnet_amd", "csrc", "*.h*"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def write_outputs(directory: str, tensors: dict) -> None:
    """``--dump-outputs``: every tensor as ``<directory>/<name>.npy`` in float32, ``DUMP_MAX_BYTES`` in all.  An array
    over its share of that budget is stored as a fixed sample of its flattened elements (indices drawn once from a
    generator seeded with the element count, ascending), so the same elements are kept in every run."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    share = DUMP_MAX_BYTES // 4 // max(len(tensors), 1)                 # elements per array
    for name, t in tensors.items():
        a = t.detach().to(torch.float32).cpu().numpy()
        if a.size > share:
            keep = np.sort(np.random.default_rng(a.size).choice(a.size, size=share, replace=False))
            a = a.reshape(-1)[keep]
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--events", type=int, default=4096,
                    help="events per GPU per step (SURVEY 8d: B in {256, 1024, 4096}, report best and B=1024: "
                         "the headline is B=4096, B=1024 is reported in other_batch_size)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--profile-steps", type=int, default=10, help="eager steps with per-op HIP events (roofline)")
    ap.add_argument("--extra-events", type=int, default=1024,
                    help="also report events/s at this many events per GPU (SURVEY 8d: B in {256,1024,4096}); 0 = skip")
    ap.add_argument("--fp32-events", type=int, default=1024,
                    help="also report the fp32 parity mode at this many events per GPU (0 = skip)")
    ap.add_argument("--overlap", action="store_true",
                    help="graph building on a second HIP stream (opt-in: dispatcher-dependent, see DESIGN.md)")
    ap.add_argument("--cpu-events", type=int, default=48)
    ap.add_argument("--cpu-steps", type=int, default=10)
    ap.add_argument("--cpu-warmup", type=int, default=3)
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / all-reduce control flow only, on CPU over gloo (no kernels, value null)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline figure: clock samples, graph ties, config-3 facts, per-op timers and "
                         "roofline, other batch size, fp32 mode, library yardsticks, CPU baseline with the parity gate")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (prediction, loss, grad, weights) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args.gpus, sys.argv[1:], args.dry_run))      # nothing above touched the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: refusing to measure a different job", file=sys.stderr)
        sys.exit(2)
    if args.dry_run:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("GN_BENCH_TEST_FAIL_RANK") == str(rank):      # test hook: this rank dies before the rendezvous
            sys.exit(3)
        run_dry(args, rank, world)
        return
    # Rehearsal knobs (one-GPU box only, never set by the driver): GN_BENCH_REHEARSE=1 puts every rank on
    # cuda:0 and exchanges gradients over gloo, to exercise the multi-rank control flow without a second GPU.
    rehearse = os.environ.get("GN_BENCH_REHEARSE") == "1"
    if rehearse:
        local = 0
    elif torch.cuda.device_count() < world:
        print(f"[bench] world size {world} but {torch.cuda.device_count()} GPU(s) visible", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local)                         # before the process group: RCCL binds to the current device
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from graphnet_amd import _lib
    from graphnet_amd.parallel import FlatGradAllReduce, broadcast_parameters
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    _lib.lib()                                           # fail loudly if the HIP library is missing

    model = build_model(args.dtype).to(dev)
    if args.overlap:
        model.backbone.set_backend(overlap=True)
    broadcast_parameters(model)
    sync = FlatGradAllReduce(model.parameters())
    # Adam(lr 1e-3, eps 1e-3) as in the reference example (easy_model.py:215-235), torch's fused multi-tensor
    # implementation (one launch instead of ~10 per step)
    try:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-3, fused=True)
    except (RuntimeError, TypeError):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, eps=1e-3)
    batch = synthetic_icecube86_batch(args.events, seed=20241016 + rank).to(dev)   # disjoint shards (weak scaling)
    n_nodes = int(batch.x.shape[0])

    def eager_step():
        sync.zero_grad()
        loss = model.shared_step(batch)
        loss.backward()
        sync()
        opt.step()
        return loss

    launch = "eager"
    step = eager_step

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Untimed ramp-up before the W warm-up steps: the first seconds of sustained load run slower (GPU clock /
    # power-state ramp and allocator growth: 10.0 ms/step with 5 warm-up steps vs 7.5 ms/step with 40), so a short
    # warm-up would time the ramp instead of the steady state - see ramp_up().
    _log(f"rank {rank}/{world}: {args.events} events = {n_nodes} pulses per GPU; ramp-up + warm-up")
    # --dump-outputs: exactly RAMP_UP_STEPS, so that the timed region starts from the same weights in every run
    ramp_max_s = 0.0 if args.dump_outputs else RAMP_UP_MAX_S if args.full else min(RAMP_UP_MAX_S, RAMP_UP_MAX_S_PLAIN)
    ramp = ramp_up(step, world, dev, RAMP_UP_STEPS, ramp_max_s)
    if rank == 0:
        _log(f"ramp-up: {ramp['steps']} steps in {ramp['seconds']:.1f} s, ms/step per block of 10: {ramp['block_ms_per_step']}")
    for _ in range(args.warmup):
        step()
    fence()
    mem0 = torch.cuda.memory_stats(dev)
    sampler = ClockSampler(dev).start() if args.full else None
    last_pred = []
    if args.dump_outputs:                            # keeps the task output of the step that ran last
        model._tasks[0].register_forward_hook(lambda _m, _i, o: last_pred.__setitem__(slice(None), [o]))
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    host_ms = []
    t0 = time.perf_counter()
    step_ev[0].record()
    for i in range(args.steps):
        th0 = time.perf_counter()
        loss = step()
        step_ev[i + 1].record()                     # one event per step on the launch stream, no synchronisation
        host_ms.append(1e3 * (time.perf_counter() - th0))
    fence()
    dt = time.perf_counter() - t0
    if sampler is not None:
        sampler.stop()
    mem1 = torch.cuda.memory_stats(dev)
    if args.dump_outputs and rank == 0:             # before anything below steps the model again
        write_outputs(args.dump_outputs, {
            "prediction": last_pred[0], "loss": loss.reshape(1), "grad": sync.flat,
            "weights": torch.cat([p.detach().reshape(-1) for p in model.parameters()])})
    step_ms = [a.elapsed_time(b) for a, b in zip(step_ev[:-1], step_ev[1:])]
    sm = sorted(step_ms)
    med = sm[len(sm) // 2]
    hm = sorted(host_ms)
    timed_region = {
        # GPU-side duration of every timed step (event to event on the launch stream): a uniformly slow clock shows as
        # min ~ median ~ max, stalls as a few steps far above the median
        "step_ms": {"min": sm[0], "median": med, "max": sm[-1], "n_slow": sum(1 for v in step_ms if v > 1.15 * med),
                    "all": [round(v, 3) for v in step_ms]},
        "host_enqueue_ms": {"min": hm[0], "median": hm[len(hm) // 2], "max": hm[-1]},
        "allocator": {k: int(mem1.get(k, 0)) - int(mem0.get(k, 0)) for k in
                      ("num_alloc_retries", "num_device_alloc", "num_device_free", "num_sync_all_streams", "num_ooms")},
        "reserved_gb": mem1.get("reserved_bytes.all.current", 0) / 1e9,
        # the step time depends on the training state: Adam steps on the one synthetic batch make the learned k-NN
        # coordinates collapse onto shared values, the graphs of layers 3-4 fill with distance ties ((k+1)-th neighbours
        # = overflow rows, hub sources) and the data-dependent kernels grow (6.4 -> 6.9 ms/step at B = 1024
        # from ~250 optimizer steps on).  Two runs compare only at the same number of steps taken before the timed region.
        "optimizer_steps_before": ramp["steps"] + args.warmup,
    }
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    if rank == 0:
        _log(f"timed region: {1e3 * dt / args.steps:.2f} ms/step" +
             ("; per-op timers, other batch sizes and modes next" if args.full else ""))
    final_loss = float(loss.detach())
    more = None
    if args.full:
        timed_region["clock"] = sampler.summary()
        timed_region["graph_ties_after"] = graph_ties(model, batch)
        more = full_measurements(args, model, sync, opt, batch, eager_step, fence, dev, rank, world, dt)

    exit_code = 0
    if rank == 0:
        out = {
            "metric": "events/sec DynEdge fwd+bwd, IceCube-86 k=8",
            "value": args.events * world * args.steps / dt, "unit": "events/s",
            "n_gpus": dist.get_world_size() if world > 1 else 1,
            "steps": args.steps, "warmup": args.warmup, "ramp_up_steps": ramp["steps"], "ramp_up": ramp,
            "timed_region": timed_region,
            "library": {"path": os.path.relpath(_lib.LIB_PATH, ROOT), "built_in_run": bool(_lib.BUILT_IN_PROCESS),
                        "so_mtime": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(os.path.getmtime(_lib.LIB_PATH))),
                        "kernel_source_hash": kernel_source_hash()},
            "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("configs[1]: DynEdge energy regression, synthetic IceCube-86 pulses "
                                    "(~150/event, 7 features), k=8, fwd+bwd+Adam" if world == 1 else
                                    f"configs[2]: configs[1] as event-batch data parallel over {world} GPUs, "
                                    "RCCL gradient all-reduce"),
                       "events_per_gpu": args.events, "global_batch": args.events * world,
                       "pulses_per_gpu": n_nodes,
                       "parallelism": f"dp{world} (event shards, one flat RCCL all-reduce)"},
            "backend": (dist.get_backend() if world > 1 else None),
            "allreduce_bytes": int(sync.flat.numel()) * 4,
            "launch": launch, "final_loss": final_loss, "full": bool(args.full),
            "outputs_dumped": bool(args.dump_outputs),
        }
        if args.full:
            out["config"]["edges_per_layer"] = more.pop("edges_per_layer")
            out.update(more)
        parity_ok = out.get("cpu_baseline", {}).get("parity", {}).get("pass", True)
        print(json.dumps(out))
        sys.stdout.flush()
        if not parity_ok:               # the in-run parity gate gates: a fast wrong answer is not a result
            print("[bench] PARITY GATE FAILED against the oracle: " + json.dumps(out["cpu_baseline"]["parity"]),
                  file=sys.stderr, flush=True)
            exit_code = 3
    if world > 1:
        dist.barrier()                  # with --full rank 0 is still measuring its yardsticks: leave together
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


def full_measurements(args, model, sync, opt, batch, eager_step, fence, dev, rank: int, world: int, dt: float):
    """``--full``, after the timed region and on the same model.  Every rank (these steps contain collectives): the
    config-3 facts, the per-op HIP-event timers over a few eager steps, the second batch size and the fp32 mode; rank 0
    then prices the roofline, measures the library yardsticks and the CPU baseline and returns the fields it adds to
    the result line (other ranks: None).  ``dt``: seconds the timed region took."""
    from graphnet_amd import ops
    n_nodes = int(batch.x.shape[0])
    # config-3 facts: replicas bitwise identical after the timed steps, cost of the exchange
    same_weights = weights_identical_across_ranks(model)
    ar_alone_us = allreduce_us(sync)
    # per-kernel durations: HIP events on the launch stream around every C-ABI op.  A graph replay has
    # no per-kernel events, so the same kernels are timed in a few eager steps right after the timed
    # region (same process, same buffers); rocprofv3 --kernel-trace of this command must agree.
    fence()
    th = time.perf_counter()
    eager_step()                                              # host time to ENQUEUE one step (no sync)
    host_issue_ms = 1e3 * (time.perf_counter() - th)
    fence()
    ops.enable_timers(True)
    ar_events = []
    prof_steps = max(1, args.profile_steps)
    for _ in range(prof_steps):
        sync.zero_grad()
        loss_p = model.shared_step(batch)
        loss_p.backward()
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        sync()                                                # flat copy-back + the ONE all-reduce of the step
        ev[1].record()
        ar_events.append(ev)
        opt.step()
    fence()
    timers = ops.timer_summary()
    detail = ops.timer_summary(detail=True)
    ops.enable_timers(False)
    ar_in_step_us = 1e3 * sum(a.elapsed_time(b) for a, b in ar_events) / prof_steps
    # second batch size (same model, same step), reported beside the headline value
    extra = None
    if args.extra_events and args.extra_events != args.events:
        extra = timed_side_run(model, sync, opt, args.extra_events, 20241016 + 1000 + rank, dev, world, fence, 30, 20)
    # fp32 parity mode (exact-f32 MFMA, fp32 storage) from the same process
    fp32 = None
    if args.fp32_events and args.dtype == "bf16":
        if rank == 0:
            _log(f"fp32 parity mode at {args.fp32_events} events per GPU")
        model.backbone.set_backend(dtype="fp32")
        fp32 = timed_side_run(model, sync, opt, args.fp32_events, 20241016 + 2000 + rank, dev, world, fence, 5, 8)
        fp32["dtype"] = "f32 (v_mfma_f32_32x32x2_f32, fp32 storage)"
        model.backbone.set_backend(dtype="bf16")
    fields = None
    if rank == 0:
        # edges of the layer-1 graph (degree k or k+1) ~ edges of every layer
        with torch.no_grad():
            t = ops.knn_graph(batch.x, [0, 1, 2], batch.batch.to(torch.int32), batch.ptr.to(torch.int32), 8)
            n_edges = int((t.nbr >= 0).sum().item()) + int(t.ovf_cnt.item())
        flops_fwd = algorithmic_flops(n_nodes, n_edges, args.events)
        flops_exec = executed_flops(n_nodes, n_edges, args.events)
        peak = PEAK_BF16_TFLOPS if args.dtype == "bf16" else PEAK_F32_TFLOPS
        # dominant op group (by HIP-event time on the launch stream) priced with ITS OWN algorithmic work:
        # MFMA groups in FLOPs (2*rows*K*N of the contraction it performs), HBM groups in bytes.
        E, N = float(n_edges), float(n_nodes)
        conv = [(19, 128, 256), (256, 336, 256), (256, 336, 256), (256, 336, 256)]       # (F_in, H1, H2)
        F0 = 19
        flops = {
            "edgeconv_fwd": sum(2 * E * h1 * h2 for _, h1, h2 in conv),
            "edgeconv_bwd": sum(2 * E * h1 * h2 for _, h1, h2 in conv),
            "edgeconv_dw2": sum(2 * E * h1 * h2 for _, h1, h2 in conv),
            # P|Q GEMMs, post MLP (2 layers), their input-gradient GEMMs, conv input gradients
            "linear_fwd": sum(2 * N * f * 2 * h1 for f, h1, _ in conv) + 2 * N * ((F0 + 1024) * 336 + 336 * 256)
                          + 2 * N * (336 * 256 + (F0 + 1024) * 336) + sum(2 * N * 2 * h1 * f for f, h1, _ in conv[1:]),
            "linear_wgrad": sum(2 * N * f * 2 * h1 for f, h1, _ in conv) + 2 * N * ((F0 + 1024) * 336 + 336 * 256),
        }
        act = 2 if args.dtype == "bf16" else 4     # bytes per stored activation element
        hbm_bytes = {   # algorithmic bytes per step of the HBM-bound groups
            "edgeconv_dq_gather": sum((E + N) * act * ((h1 + 31) // 32 * 32) for _, h1, _ in conv),
            "knn_graph": 4 * (N * 3 * 4 + N * 9 * 4),
            "colsum": sum(N * 4 * h1 for _, h1, _ in conv) + N * 4 * (336 + 256),
            "segment_pool_fwd": N * 256 * 4, "segment_pool_bwd": N * 256 * (4 + act),
        }
        # candidates: ONE kernel shape each (the op groups that mix shapes list them in `detail`: conv 1 is 128 wide,
        # conv 2-4 are 336 wide; the GEMM groups hold five different contractions) - this is the duration a rocprofv3
        # kernel trace reports for that kernel
        cands = {}
        for gname, tv in timers.items():
            shapes = {k: v for k, v in detail.items() if k.startswith(gname + "[")}
            if shapes:
                cands.update({k: (gname, v) for k, v in shapes.items()})
            else:
                cands[gname] = (gname, tv)
        kernel_shape, (name, (launches, ms)) = (max(cands.items(), key=lambda kv: kv[1][1][1]) if cands
                                                else ("none", ("none", (1, 0.0))))
        per_launch_ms = ms / max(launches, 1)
        lps = launches / prof_steps
        if name in flops:
            bound, unit = "mfma", "TFLOP/s"
            if "[" in kernel_shape:
                a_, b_ = (int(v) for v in kernel_shape[len(name) + 1:-1].split("x"))
                if name.startswith("edgeconv"):        # [H1p x H2]: contraction over the edge rows
                    h1 = next(h for _, h, _ in conv if (h + 31) // 32 * 32 == a_)
                    achieved = 2 * E * h1 * b_ / (per_launch_ms * 1e-3) / 1e12
                else:                                  # [K x N]: one GEMM over the N pulse rows
                    achieved = 2 * N * a_ * b_ / (per_launch_ms * 1e-3) / 1e12
            else:
                achieved = flops[name] / lps / (per_launch_ms * 1e-3) / 1e12
        else:
            bound, unit, peak = "hbm", "GB/s", 8000.0
            achieved = hbm_bytes.get(name, 0.0) / lps / (per_launch_ms * 1e-3) / 1e9
        # HBM traffic per launch of that group: NOT measured in this run (PMC counters need rocprofv3 passes of
        # their own) - read from the committed summary of the `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` passes
        # over this same command (FETCH_SIZE doubled as the gfx950 guide prescribes)
        traffic, traffic_source = None, None
        try:
            tj = json.load(open(os.path.join(ROOT, TRAFFIC_FILE)))
            if tj.get(name, {}).get("events_per_gpu", 1024) == args.events:      # measured on this workload only
                if tj.get("_kernel_source_hash") == kernel_source_hash():
                    traffic = tj.get(name, {}).get("bytes_per_launch")
                    traffic_source = f"from_file: {TRAFFIC_FILE}@{tj.get('_commit', 'unknown')} (kernel sources unchanged)"
                else:       # the kernels changed after the counters were read: do not pass the number on
                    traffic_source = (f"stale: {TRAFFIC_FILE} was measured on kernel sources "
                                      f"{tj.get('_kernel_source_hash')}, this run has {kernel_source_hash()}")
        except Exception:
            pass
        fields = {
            "edges_per_layer": n_edges,
            "allreduce_us_per_step": ar_in_step_us if world > 1 else 0.0,
            "allreduce_alone_us": ar_alone_us,
            "weights_identical_across_ranks": same_weights,
            "roofline": {"bound": bound, "kernel": kernel_shape, "achieved": achieved, "peak": peak, "unit": unit,
                         "frac": achieved / peak, "traffic": traffic, "traffic_source": traffic_source,
                         "launch_ms": per_launch_ms, "launches_per_step": lps},
            "group_tflops": {k: flops[k] / (timers[k][1] / prof_steps * 1e-3) / 1e12 for k in flops if k in timers},
            # whole step against the MFMA peak, per GPU.  Two prices: the reference formulation's FLOPs (SURVEY.md 8d:
            # what PyG would execute for the same result) and the FLOPs this path really executes (P|Q split)
            "path_roofline": {"reference_formulation_tflop_per_step": 3.0 * flops_fwd / 1e12,
                              "reference_formulation_tflops_equiv": 3.0 * flops_fwd * args.steps / dt / 1e12,
                              "reference_formulation_frac": 3.0 * flops_fwd * args.steps / dt / 1e12 / peak,
                              "executed_tflop_per_step": flops_exec / 1e12,
                              "executed_tflops": flops_exec * args.steps / dt / 1e12,
                              "executed_frac": flops_exec * args.steps / dt / 1e12 / peak,
                              "note": "per GPU; executed_frac is the MFMA utilisation of the step"},
            "phase_ms_per_step": {k: v[1] / prof_steps for k, v in sorted(timers.items(), key=lambda kv: -kv[1][1])},
            # the same HIP-event pairs keyed by kernel shape ([H1p x H2] of an edge kernel, [K x N] of a GEMM): (launches per
            # step, ms per launch)
            "kernel_shape_ms": {k: [v[0] / prof_steps, v[1] / max(v[0], 1)]
                                for k, v in sorted(detail.items(), key=lambda kv: -kv[1][1])},
            "host_issue_ms": host_issue_ms,
            "measured_peaks": (_log("yardsticks: library GEMM, device copy"), measured_peaks(dev))[1],
            "other_batch_size": extra,
            "fp32": fp32,
        }
        if world == 1 and not args.no_cpu_baseline:
            fields["cpu_baseline"] = cpu_baseline(args.cpu_events, args.cpu_steps, args.cpu_warmup, parity_model=model)
    return fields


if __name__ == "__main__":
    main()
