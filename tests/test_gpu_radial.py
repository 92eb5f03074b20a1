"""``gn_radius_graph`` / ``RadialEdges`` on the device against the numpy fp32 brute force of ``radial_reference.py``
(pinned against a k-d tree by tests/test_radial_host.py).

Every table comparison is exact (``torch.equal``): the arithmetic is specified operation by operation, the rule is the
strict ``d2 < r2`` and the cap keeps the smallest ``(d2, j)``, so there is nothing to tolerate."""
import numpy as np
import pytest
import torch

from radial_reference import edge_index_of, ptr_of, radius_table

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _device_table(x, ptr, r, cap, cols=(0, 1, 2)):
    from graphnet_amd import ops
    ptr32 = ptr.to(torch.int32).to(DEV)
    n = int(x.shape[0])
    batch32 = ops.ptr_to_batch(ptr32, n) if n else torch.zeros(0, dtype=torch.int32, device=DEV)
    t = ops.radius_graph(x, list(cols), r, batch32, ptr32, cap)
    assert t.ovf is None and t.event_ptr is ptr32 and t.nbr.is_contiguous()                  # the strict form
    assert tuple(t.nbr.shape) == (int(x.shape[0]), t.K) and tuple(t.deg.shape) == (int(x.shape[0]),)
    return t


def _check(t, exp_nbr, exp_deg, cap):
    """The device table is the reference's, cut to the width the graph needs; ``deg`` is the uncapped count."""
    assert torch.equal(t.deg.cpu(), exp_deg)
    K = max(1, min(cap, int(exp_deg.max()) if exp_deg.numel() else 0))
    assert t.K == K
    assert torch.equal(t.nbr.cpu(), exp_nbr[:, :K])
    assert bool((exp_nbr[:, K:] == -1).all())


# ------------------------------------------------------------------------------ 1. tile / chunk / cap boundaries
SIZES = [1, 2, 3, 9, 63, 64, 65, 256, 257, 600, 1100]


@pytest.fixture(scope="module")
def shapes_batch():
    gen = torch.Generator().manual_seed(20)
    x = torch.randn(sum(SIZES), 3, generator=gen)
    return x, ptr_of(SIZES), x.to(DEV), {}


def _expected(shapes_batch, r, cap):
    x, ptr, _, cache = shapes_batch
    if (r, cap) not in cache:
        cache[(r, cap)] = radius_table(x, ptr, [0, 1, 2], r, cap)
    return cache[(r, cap)]


@pytest.mark.parametrize("cap", [1, 8, 32])
@pytest.mark.parametrize("r", [0.25, 0.5, 1.0])
def test_shapes_where_the_kernel_can_go_wrong(shapes_batch, r, cap):
    _, ptr, xd, _ = shapes_batch
    exp_nbr, exp_deg = _expected(shapes_batch, r, cap)
    _check(_device_table(xd, ptr, r, cap), exp_nbr, exp_deg, cap)


def test_the_input_exercises_both_paths_and_both_sides_of_the_cap(shapes_batch):
    """What the reference alone says about the input above (no device code): the figures the cases rely on."""
    deg = {r: _expected(shapes_batch, r, 32)[1] for r in (0.25, 0.5, 1.0)}
    assert int((deg[0.25] == 0).sum()) == 1247 and deg[0.25].numel() == sum(SIZES) == 2420 and int((deg[0.25] > 32).sum()) == 0
    assert (int((deg[0.5] > 32).sum()), int((deg[0.5] == 32).sum()), int((deg[0.5] == 33).sum())) == (28, 9, 12)
    assert int((deg[1.0] > 32).sum()) == 1354


# ------------------------------------------------------------------------------ 2. ties and strictness
@pytest.mark.parametrize("cap", [8, 32])
@pytest.mark.parametrize("r", [1.0, 2.0])
def test_ties_and_strictness_on_an_integer_grid(r, cap):
    gen = torch.Generator().manual_seed(5)
    sizes = [300, 90]
    n = sum(sizes)
    x = torch.randint(0, 4, (n, 3), generator=gen).float()
    x[40:80] = x[40]                                           # forty coincident pulses, d2 = 0: more than any cap
    x[7, 1] = float("nan")
    x[11, 2] = float("inf")
    ptr = ptr_of(sizes)
    exp_nbr, exp_deg = radius_table(x, ptr, [0, 1, 2], r, cap)
    t = _device_table(x.to(DEV), ptr, r, cap)
    _check(t, exp_nbr, exp_deg, cap)
    got = t.nbr.cpu()
    for bad in (7, 11):                                        # no neighbours, nobody's neighbour
        assert bool((got[bad] == -1).all()) and not bool((got == bad).any()) and int(t.deg[bad]) == 0
    assert not bool((got == torch.arange(n, dtype=torch.int32).unsqueeze(1)).any())          # no self loops
    big = torch.where(got >= 0, got, torch.full_like(got, 2 ** 30))
    assert bool((big[:, 1:] > big[:, :-1]).logical_or(big[:, 1:] == 2 ** 30).all())           # every group ascends
    if r == 1.0:                                               # d2 == r2 is out: only coincident pulses connect
        ei = edge_index_of(got)
        assert bool((x[ei[0]] == x[ei[1]]).all()) and ei.shape[1] > 0
        assert bool((got[40:80, :min(cap, 39)] >= 0).all())


# ------------------------------------------------------------------------------ 3. columns and row pitch
@pytest.mark.parametrize("case", ["permuted", "two_columns", "strided"])
def test_columns_and_row_pitch(case):
    gen = torch.Generator().manual_seed(31)
    sizes = [5, 130, 70, 300]
    n = sum(sizes)
    ptr = ptr_of(sizes)
    x = torch.randn(n, 7, generator=gen)
    cols, r = [4, 0, 2], 0.6
    if case == "two_columns":
        cols, r = [6, 1], 0.3
    if case == "strided":
        big = torch.randn(n, 12, generator=gen).to(DEV)
        xd = big[:, 3:10]                                      # row pitch 12, seven columns, not contiguous
        assert not xd.is_contiguous()
        x = xd.cpu().contiguous()
    else:
        xd = x.to(DEV)
    exp_nbr, exp_deg = radius_table(x, ptr, cols, r, 16)
    assert int((exp_deg > 16).sum()) > 0 and int((exp_deg == 0).sum()) > 0
    _check(_device_table(xd, ptr, r, 16, cols), exp_nbr, exp_deg, 16)


# ------------------------------------------------------------------------------ 4. empty neighbourhoods
def test_empty_neighbourhoods_and_an_empty_batch():
    sizes = [70, 1, 300]
    n = sum(sizes)
    x = torch.zeros(n, 3)
    x[:, 0] = torch.arange(n, dtype=torch.float32) * 2.0       # every pair at least 2 apart
    t = _device_table(x.to(DEV), ptr_of(sizes), 1.0, 32)
    assert t.K == 1 and bool((t.nbr == -1).all()) and bool((t.deg == 0).all())
    ei = t.edge_index()
    assert tuple(ei.shape) == (2, 0) and ei.dtype == torch.int64
    t = _device_table(torch.zeros(0, 3, device=DEV), ptr_of([0]), 1.0, 32)
    assert t.K == 1 and tuple(t.nbr.shape) == (0, 1)


# ------------------------------------------------------------------------------ 5. the edge definition on device
def test_edge_definition_on_a_device_batch_and_on_a_single_event():
    import graphnet_amd as g
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    b = synthetic_icecube86_batch(6, seed=17)
    x, ptr = b.x.clone(), b.ptr.clone()
    ed = g.RadialEdges(0.2)
    out = ed(b.to(DEV))
    assert out.edge_index.is_cuda and out.edge_index.dtype == torch.int64
    exp_nbr, exp_deg = radius_table(x, ptr, [0, 1, 2], 0.2, 32)
    assert int((exp_deg > 32).sum()) == 15 and int(exp_deg.max()) == 44        # the cap is at work on this batch
    assert torch.equal(out.edge_index.cpu(), edge_index_of(exp_nbr))
    lo, hi = int(ptr[2]), int(ptr[3])
    one = ed(g.Data(x=x[lo:hi].to(DEV)))                       # no `batch`: one event
    exp = edge_index_of(radius_table(x[lo:hi], ptr_of([hi - lo]), [0, 1, 2], 0.2, 32)[0])
    assert torch.equal(one.edge_index.cpu(), exp)


# ------------------------------------------------------------------------------ 6. the backbone honours the record
def _strip_record(b):
    from graphnet_amd.graphs import RADIAL_RECORD
    for name in RADIAL_RECORD:
        b[name] = None
    return b


@pytest.mark.parametrize("path", ["collate", "batch_from_raw"])
def test_dynedge_builds_the_recorded_graph(path):
    import graphnet_amd as g
    from graphnet_amd.graphs import radial_record
    from graphnet_amd.synthetic import FEATURES_ICECUBE86, synthetic_icecube86_raw
    r = 0.15
    raw, rptr, _ = synthetic_icecube86_raw(6, seed=23)
    events = [raw[rptr[i]:rptr[i + 1]].astype(np.float64) for i in range(6)]
    gd = g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86, edge_definition=g.RadialEdges(r))
    if path == "collate":
        b = g.collate_fn([gd(e, FEATURES_ICECUBE86) for e in events])      # on the CPU: no edges, the record
        assert "edge_index" not in b.keys()
        b = b.to(DEV)
    else:
        b = gd.batch_from_raw(events, FEATURES_ICECUBE86, device=DEV)
    rec = radial_record(b)
    assert (float(np.float32(rec[0])), rec[1], rec[2]) == (float(np.float32(r)), [0, 1, 2], 32)
    exp_nbr, exp_deg = radius_table(b.x.cpu(), b.ptr.cpu(), [0, 1, 2], rec[0], 32)
    assert int(exp_deg.max()) == 16                                         # nothing over the cap, a table 16 wide
    bounds = b.ptr.cpu().tolist()
    assert all(int(exp_deg[lo:hi].sum()) > 0 for lo, hi in zip(bounds[:-1], bounds[1:]))      # every event has edges
    exp_ei = edge_index_of(exp_nbr)

    torch.manual_seed(4)
    # pooled output: without pooling schemes a DynEdge has no one-call path at all
    m = g.DynEdge(7, dynedge_layer_sizes=[(128, 256), (336, 256)],
                  global_pooling_schemes=["min", "max", "mean", "sum"]).to(DEV)
    m.set_backend(dtype="fp32")
    assert m._stepper(7) is not None                                        # this configuration takes the one-call path
    with torch.no_grad():
        out_step = m(b)                                                     # the one-call path
        out_trace, trace = m(b, return_trace=True)                          # the per-op path
        assert torch.equal(trace["graphs"][0].edge_index().cpu(), exp_ei)
        explicit = g.Batch(x=b.x, edge_index=exp_ei.to(DEV))
        explicit.ptr, explicit.batch, explicit.n_pulses = b.ptr, b.batch, b.n_pulses
        assert radial_record(explicit) is None
        ref_step = m(explicit)
        ref_trace, _ = m(explicit, return_trace=True)
    assert torch.equal(out_step, ref_step) and torch.equal(out_trace, ref_trace)
    assert torch.equal(out_step, ref_trace)
    # and it is not the backbone's own k-NN graph that was built
    with torch.no_grad():
        assert not torch.equal(m(_strip_record(b)), out_step)


# ------------------------------------------------------------------------------ 7. parity on a variable-degree graph
def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def norm_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _pair(oracle, F=7, seed=20241016, **kw):
    import graphnet_amd as g
    torch.manual_seed(seed)
    ref = oracle.StandardModelOracle(F, **kw)
    m = g.StandardModel(
        graph_definition=g.KNNGraph(g.IceCube86()),
        backbone=g.DynEdge(F, **kw),
        tasks=[g.EnergyReconstruction(hidden_size=128, loss_function=g.LogCoshLoss(),
                                      transform_prediction_and_target=torch.log10)],
        optimizer_kwargs={"lr": 1e-3, "eps": 1e-3},
    )
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


@pytest.mark.parametrize("cap", [32, 8])
@pytest.mark.parametrize("dtype,tol,gtol", [("fp32", 1e-4, 1e-3), ("bf16", 2e-2, 2e-2)])     # SURVEY.md 8d gates
def test_full_model_teacher_forced_on_a_radius_graph(oracle, dtype, tol, gtol, cap):
    """``test_gpu_model.py::test_full_model_teacher_forced`` with the layer-1 graph of ``RadialEdges(0.15)``: a table 18
    wide (8 with ``max_num_neighbours=8``, where capped centres occur), mostly padding, with isolated centres."""
    import graphnet_amd as g
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    b = synthetic_icecube86_batch(16, seed=77)
    exp_nbr, exp_deg = radius_table(b.x, b.ptr, [0, 1, 2], 0.15, cap)
    bounds = b.ptr.tolist()
    assert int(exp_deg.max()) == 18 and int((exp_deg == 0).sum()) == 317 and exp_deg.numel() == 2569
    assert min(int(exp_deg[lo:hi].sum()) for lo, hi in zip(bounds[:-1], bounds[1:])) >= 76
    assert (int((exp_deg > cap).sum()) > 0) == (cap == 8)
    b = g.RadialEdges(0.15, max_num_neighbours=cap)(b)          # on the CPU: the record, the backbone builds the graph
    kw = dict(global_pooling_schemes=["min", "max", "mean", "sum"])
    ref, m = _pair(oracle, **kw)
    m.backbone.set_backend(dtype=dtype)
    latent, trace = m.backbone(b.to(DEV), return_trace=True)
    pred = m._tasks[0](latent)
    loss = m._tasks[0].compute_loss(pred, {"energy": b.energy})
    loss.backward()

    bc = b.to("cpu")
    assert trace["graphs"][0].K == min(cap, 18) and trace["graphs"][0].ovf is None
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], edge_index_of(exp_nbr))
    lat_o, tr_o = ref.backbone(bc.x, forced[0], bc.batch, bc.n_pulses, return_trace=True, forced_edges=forced)
    errs = {"global_variables": rel_err(trace["global_variables"], tr_o["global_variables"])}
    for l in range(5):
        w = tr_o["conv_out"][l].shape[1]
        errs[f"conv_out[{l}]"] = rel_err(trace["conv_out"][l][:, :w], tr_o["conv_out"][l].detach())
    errs["post"] = rel_err(trace["post"], tr_o["post"].detach())
    errs["latent"] = rel_err(latent, lat_o.detach())
    pred_o = oracle.energy_reconstruction(lat_o, ref._affine)
    loss_o = oracle.log_cosh_loss(pred_o, torch.log10(bc.energy).unsqueeze(1))
    loss_o.backward()
    errs["pred"] = rel_err(pred, pred_o.detach())
    errs["loss"] = abs(float(loss) - float(loss_o)) / abs(float(loss_o))
    go = dict(ref.named_parameters())
    # bf16: gate on the Frobenius-norm error (single relu gates may flip); fp32: max-abs
    gerrs = {k: (rel_err(p.grad, go[k].grad) if dtype == "fp32" else norm_err(p.grad, go[k].grad))
             for k, p in m.named_parameters() if p.grad is not None}
    print(f"radial parity {dtype} cap={cap}: activations {errs} gradients max {max(gerrs.values()):.3e}")
    assert errs.pop("global_variables") < 1e-5
    for name, e in errs.items():
        assert e < tol, f"{dtype}: {name}: {e}"
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert gerrs[k] < gtol, f"{dtype}: grad {k}: {gerrs[k]}"
