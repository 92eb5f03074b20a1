"""``gn_percentile_clusters`` / ``PercentileClusters`` on the device against the loop-per-cluster restatement of
``percentile_reference.py`` (pinned against the reference's recorded results by tests/test_percentile_host.py).

Every comparison is exact, NaN == NaN, but for the counts column: the device ``log10`` is not numpy's, so there the fp32
bit patterns may differ by one (``same_but_counts``)."""
import numpy as np
import pytest
import torch

import percentile_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PCT = [0, 10, 50, 90, 100]


def _device(x, ptr, cl, sm, pct=PCT, add_counts=True, **kw):
    from graphnet_amd import ops
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    ptr32 = torch.as_tensor(np.asarray(ptr), dtype=torch.int32).to(DEV)
    nodes, node_ptr = ops.percentile_clusters(xd, ptr32, cl, sm, pct, add_counts, **kw)
    W = len(cl) + len(sm) * len(pct) + (1 if add_counts else 0)
    assert nodes.dtype == torch.float32 and node_ptr.dtype == torch.int32 and nodes.is_cuda
    assert tuple(node_ptr.shape) == (len(ptr),) and tuple(nodes.shape) == (int(node_ptr[-1]), W)
    return nodes.cpu().numpy(), node_ptr.cpu().numpy()


def _check(x, ptr, cl, sm, pct=PCT, add_counts=True, xd=None, **kw):
    exp, exp_ptr = R.cluster_batch(x, ptr, cl, sm, pct, add_counts)
    got, got_ptr = _device(x if xd is None else xd, ptr, cl, sm, pct, add_counts, **kw)
    assert np.array_equal(got_ptr, exp_ptr)
    assert R.same_but_counts(got, exp, add_counts)
    return exp, exp_ptr


# ------------------------------------------------------------------------------ 1. shapes where the kernel can go wrong
@pytest.fixture(scope="module")
def shapes():
    x, ptr = R.shapes_batch()
    return x, ptr, R.cluster_batch(x, ptr, [0, 1, 2], [3, 4, 5], PCT)


def test_shapes_where_the_kernel_can_go_wrong(shapes):
    x, ptr, (exp, exp_ptr) = shapes
    got, got_ptr = _device(x, ptr, [0, 1, 2], [3, 4, 5])
    assert np.array_equal(got_ptr, exp_ptr)
    assert R.same_but_counts(got, exp)


def test_the_input_has_single_pulse_clusters_and_large_ones(shapes):
    """What the restatement alone says about the input above (no device code): the figures the case relies on."""
    x, ptr, (exp, exp_ptr) = shapes
    assert np.diff(exp_ptr).tolist() == [1, 1, 1, 2, 15, 16, 15, 62, 64, 148, 270, 503]
    assert (len(exp), len(x)) == (1098, 4469)
    counts = np.rint(10.0 ** exp[:, -1].astype(np.float64)).astype(np.int64)
    assert int(counts.sum()) == 4469 and int((counts == 1).sum()) == 100 and int(counts.max()) == 11
    assert bool((exp[counts == 1, -1] == 0).all())


# ------------------------------------------------------------------------------ 2. extremes of clustering
def test_one_cluster_and_all_distinct():
    gen = np.random.default_rng(3)
    x = gen.standard_normal((600, 6)).astype(np.float32)
    one = x.copy()
    one[:, :3] = one[0, :3]
    exp, exp_ptr = _check(one, [0, 600], [0, 1, 2], [3, 4, 5])
    assert exp_ptr.tolist() == [0, 1]
    for s in range(3):                                         # every percentile interpolates across the whole event
        assert np.allclose(exp[0, 3 + 5 * s:8 + 5 * s], np.percentile(one[:, 3 + s].astype(np.float64), PCT), rtol=1e-6)
    got, got_ptr = _device(x, [0, 600], [0, 1, 2], [3, 4, 5])
    assert got_ptr.tolist() == [0, 600]
    order = np.lexsort((x[:, 0], x[:, 1], x[:, 2]))
    assert np.array_equal(got[:, :3], x[order, :3])
    for s in range(3):                                         # every percentile is the value itself
        assert np.array_equal(got[:, 3 + 5 * s:8 + 5 * s], np.repeat(x[order, 3 + s][:, None], 5, axis=1))
    assert bool((got[:, -1].view(np.int32) == 0).all())        # log10(1), exactly +0.0


def test_an_event_above_the_lds_limit_between_small_ones():
    from graphnet_amd import _lib
    big = int(_lib.lib().gn_percentile_lds_max()) + 1
    gen = np.random.default_rng(11)
    sizes = [70, big, 9]
    x = np.concatenate([R.make_event(gen, n) for n in sizes], axis=0)
    exp, exp_ptr = _check(x, np.cumsum([0] + sizes), [0, 1, 2], [3, 4, 5])
    assert int(exp_ptr[2] - exp_ptr[1]) > 900                  # the large event keeps many clusters


def test_event_sizes_on_both_sides_of_every_kernel_threshold():
    """512 / 513: a power of two and one more (the sort pads an event to the next power of two); ``gn_percentile_lds_max()``:
    the largest event sorted in LDS (one more pulse is the case above); 1024 = one full batch of four pairs per thread."""
    from graphnet_amd import _lib
    gen = np.random.default_rng(12)
    sizes = [513, 511, 512, int(_lib.lib().gn_percentile_lds_max()), 3, 1024, 1025]
    x = np.concatenate([R.make_event(gen, n) for n in sizes], axis=0)
    _check(x, np.cumsum([0] + sizes), [0, 1, 2], [3, 4, 5])
    _check(x[513:513 + 511], [0, 200, 511], [0, 1, 2], [3, 4, 5])
    _check(x[:513], [0, 513], [0, 1, 2], [3, 4, 5])


# ------------------------------------------------------------------------------ 3. ties and specials
def test_ties_signed_zeros_nan_and_inf():
    x = np.concatenate([R.grid_event(cluster_nan=True), R.grid_event()], axis=0)
    exp, exp_ptr = _check(x, [0, 300, 600], [0, 1, 2], [3, 4, 5])
    first = exp[:exp_ptr[1]]
    assert np.isnan(first[-1, 2]) and not np.isnan(first[:-1, :3]).any()       # the NaN-keyed pulses: one cluster, last
    assert int(np.rint(10.0 ** float(first[-1, -1]))) == 3
    assert int(np.rint(10.0 ** exp[:, -1].astype(np.float64)).max()) >= 40     # the forty coincident pulses
    assert np.isnan(exp[:, 3:-1]).any() and np.isinf(exp[:, 3:-1]).any()
    zeros = x[:300][(x[:300, 0] == 0)]
    assert np.signbit(zeros[:, 0]).any() and not np.signbit(zeros[:, 0]).all()  # -0.0 and +0.0 are both in the input


# ------------------------------------------------------------------------------ 4. columns and row pitch
@pytest.mark.parametrize("case", ["permuted", "two_columns", "one_column", "P1", "P16", "no_counts", "strided", "out_pitch"])
def test_columns_and_row_pitch(case):
    gen = np.random.default_rng(31)
    sizes = [5, 130, 70, 300]
    ptr = np.cumsum([0] + sizes)
    x = np.concatenate([R.make_event(gen, n, F=7, dup=3) for n in sizes], axis=0)
    x[:, [4, 1]] = x[:, [1, 4]]                               # duplicated positions in columns 0, 4, 2
    cl, pct, add_counts, xd, kw = [4, 0, 2], PCT, True, None, {}
    if case == "two_columns":
        cl = [2, 0]
    elif case == "one_column":
        cl = [1]
        x[:, 1] = np.round(x[:, 1] * 2)
    elif case == "P1":
        pct = [37.5]
    elif case == "P16":
        pct = [0, 1, 5, 10, 20, 25, 30, 40, 50, 60, 70, 75, 80, 90, 99, 100]
    elif case == "no_counts":
        add_counts = False
    elif case == "strided":
        big = torch.randn(len(x), 12, generator=torch.Generator().manual_seed(1))
        big[:, 3:10] = torch.from_numpy(x)
        xd = big.to(DEV)[:, 3:10]                             # row pitch 12, seven columns, not contiguous
        assert not xd.is_contiguous()
    elif case == "out_pitch":
        kw = {"out_pitch": 40}
    sm = [c for c in range(7) if c not in cl]
    exp, exp_ptr = _check(x, ptr, cl, sm, pct, add_counts, xd=xd, **kw)
    assert 1 < len(exp) < len(x)


# ------------------------------------------------------------------------------ 5. empty batch, empty event
def test_an_empty_batch_and_an_empty_event_in_the_middle():
    got, got_ptr = _device(np.zeros((0, 6), dtype=np.float32), [0], [0, 1, 2], [3, 4, 5])
    assert got.shape == (0, 19) and got_ptr.tolist() == [0]
    got, got_ptr = _device(np.zeros((0, 6), dtype=np.float32), [0, 0, 0], [0, 1, 2], [3, 4, 5])
    assert got.shape == (0, 19) and got_ptr.tolist() == [0, 0, 0]
    gen = np.random.default_rng(8)
    sizes = [40, 0, 0, 90, 0]
    x = np.concatenate([R.make_event(gen, n) for n in sizes if n], axis=0)
    exp, exp_ptr = _check(x, np.cumsum([0] + sizes), [0, 1, 2], [3, 4, 5])
    assert exp_ptr[1] == exp_ptr[2] == exp_ptr[3] and exp_ptr[4] == exp_ptr[5] == len(exp)


# ------------------------------------------------------------------------------ 6. host path == device path
def _raw_events(n_events=6, seed=23):
    from graphnet_amd.synthetic import synthetic_icecube86_raw
    raw, rptr, energy = synthetic_icecube86_raw(n_events, seed=seed)
    return [raw[rptr[i]:rptr[i + 1]].astype(np.float64) for i in range(n_events)], energy


def test_host_path_and_device_path_agree():
    import graphnet_amd as g
    from graphnet_amd.synthetic import FEATURES_ICECUBE86
    events, _ = _raw_events()
    det = g.IceCube86()
    xs = [det(torch.tensor(e, dtype=torch.float32), FEATURES_ICECUBE86) for e in events]      # standardised on the host
    nd = g.PercentileClusters(["dom_x", "dom_y", "dom_z"], PCT, input_feature_names=FEATURES_ICECUBE86)
    host = [nd(x)[0].x for x in xs]
    assert all(h.dtype == torch.float32 and not h.is_cuda for h in host)
    ptr = torch.tensor(np.cumsum([0] + [len(x) for x in xs]), dtype=torch.int32)
    nodes, node_ptr = nd.cluster_batch(torch.cat(xs).to(DEV), ptr.to(DEV))
    assert node_ptr.cpu().tolist() == np.cumsum([0] + [len(h) for h in host]).tolist()
    assert R.same_but_counts(nodes.cpu().numpy(), torch.cat(host).numpy())
    one = nd(xs[2].to(DEV))[0].x                                # a device tensor without ptr: one event
    assert one.is_cuda and R.same_but_counts(one.cpu().numpy(), host[2].numpy())


# ------------------------------------------------------------------------------ 7. batch_from_raw
def _clustered_and_pulse_batches(pct):
    import graphnet_amd as g
    from graphnet_amd.synthetic import FEATURES_ICECUBE86
    events, energy = _raw_events()
    xyz = ["dom_x", "dom_y", "dom_z"]
    gd = g.KNNGraph(g.IceCube86(), node_definition=g.PercentileClusters(xyz, pct), input_feature_names=FEATURES_ICECUBE86)
    b = gd.batch_from_raw(events, FEATURES_ICECUBE86, truth={"energy": energy}, device=DEV)
    pulses = g.KNNGraph(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86).batch_from_raw(events, FEATURES_ICECUBE86, device=DEV)
    return gd, b, pulses, events


def test_batch_from_raw_clusters_the_standardised_batch():
    gd, b, pulses, events = _clustered_and_pulse_batches([10, 50, 90])
    assert gd.nb_outputs == 3 + 4 * 3 + 1 == int(b.x.shape[1])
    exp, exp_ptr = R.cluster_batch(pulses.x.cpu().numpy(), pulses.ptr.cpu().numpy(), [0, 1, 2], [3, 4, 5, 6], [10, 50, 90])
    assert b.x.dtype == torch.float32 and R.same_but_counts(b.x.cpu().numpy(), exp)
    assert b.ptr.dtype == torch.int64 and b.ptr.cpu().tolist() == exp_ptr.tolist()
    assert b.n_pulses.cpu().tolist() == [len(e) for e in events] == pulses.n_pulses.cpu().tolist()
    assert b.batch.dtype == torch.int64
    assert b.batch.cpu().tolist() == np.repeat(np.arange(len(events)), np.diff(exp_ptr)).tolist()
    assert len(exp) < int(pulses.x.shape[0]) and int(np.diff(exp_ptr).min()) >= 2
    assert b.knn_k == 8 and b.knn_columns == [0, 1, 2] and b.num_graphs == len(events)


def test_batch_from_raw_refuses_a_node_definition_it_cannot_build():
    import graphnet_amd as g
    from graphnet_amd.synthetic import FEATURES_ICECUBE86

    class Other(g.graphs.NodeDefinition):
        def _define_output_feature_names(self, names):
            return names

        def _construct_nodes(self, x):
            return g.Data(x=x)

    events, _ = _raw_events(2)
    with pytest.raises(NotImplementedError, match="Other"):
        g.KNNGraph(g.IceCube86(), node_definition=Other(), input_feature_names=FEATURES_ICECUBE86).batch_from_raw(
            events, FEATURES_ICECUBE86, device=DEV)


# ------------------------------------------------------------------------------ 8. the backbone on clustered nodes
def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_dynedge_on_clustered_nodes_teacher_forced(oracle):
    """``test_gpu_radial.py::test_full_model_teacher_forced_on_a_radius_graph`` on DOM-level nodes, fp32: nothing
    downstream may assume ``n_pulses[e] == ptr[e + 1] - ptr[e]``."""
    import graphnet_amd as g
    gd, b, pulses, events = _clustered_and_pulse_batches([50])
    F = gd.nb_outputs
    assert F == 8 and int(b.x.shape[0]) < int(pulses.x.shape[0])
    assert not torch.equal(b.n_pulses.cpu().to(torch.int64), (b.ptr[1:] - b.ptr[:-1]).cpu())
    kw = dict(global_pooling_schemes=["min", "max", "mean", "sum"])
    torch.manual_seed(20241016)
    ref = oracle.StandardModelOracle(F, **kw)
    m = g.StandardModel(
        graph_definition=gd, backbone=g.DynEdge(F, **kw),
        tasks=[g.EnergyReconstruction(hidden_size=128, loss_function=g.LogCoshLoss(),
                                      transform_prediction_and_target=torch.log10)],
        optimizer_kwargs={"lr": 1e-3, "eps": 1e-3},
    )
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV)
    m.backbone.set_backend(dtype="fp32")
    assert m.backbone._stepper(F) is not None                  # this configuration takes the one-call path
    with torch.no_grad():
        out_step = m.backbone(b)
        out_trace, _ = m.backbone(b, return_trace=True)
    assert torch.equal(out_step, out_trace)                    # one call and per-op: bit for bit

    latent, trace = m.backbone(b, return_trace=True)
    pred = m._tasks[0](latent)
    loss = m._tasks[0].compute_loss(pred, {"energy": b.energy})
    loss.backward()
    x, batch, n_pulses, energy = b.x.cpu(), b.batch.cpu(), b.n_pulses.cpu(), b.energy.cpu()
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    lat_o, tr_o = ref.backbone(x, forced[0], batch, n_pulses, return_trace=True, forced_edges=forced)
    errs = {"global_variables": rel_err(trace["global_variables"], tr_o["global_variables"])}
    for l in range(5):
        w = tr_o["conv_out"][l].shape[1]
        errs[f"conv_out[{l}]"] = rel_err(trace["conv_out"][l][:, :w], tr_o["conv_out"][l].detach())
    errs["post"] = rel_err(trace["post"], tr_o["post"].detach())
    errs["latent"] = rel_err(latent, lat_o.detach())
    pred_o = oracle.energy_reconstruction(lat_o, ref._affine)
    loss_o = oracle.log_cosh_loss(pred_o, torch.log10(energy).unsqueeze(1))
    loss_o.backward()
    errs["pred"] = rel_err(pred, pred_o.detach())
    errs["loss"] = abs(float(loss.detach()) - float(loss_o.detach())) / abs(float(loss_o.detach()))
    go = dict(ref.named_parameters())
    gerrs = {k: rel_err(p.grad, go[k].grad) for k, p in m.named_parameters() if p.grad is not None}
    print(f"clustered parity fp32: activations {errs} gradients max {max(gerrs.values()):.3e}")
    for name, e in errs.items():                               # SURVEY.md 8d gates, fp32
        assert e < 1e-4, f"{name}: {e}"
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert gerrs[k] < 1e-3, f"grad {k}: {gerrs[k]}"
