"""GPU: ``gn_icemix_nodes`` / ``IceMixNodes`` on the device against the restatement of the contract
(``icemix_reference.py``).  Exact: ``out_ptr``, ``ids`` and every row bit for bit, the two fp64-derived ice columns
included, NaN equal to NaN."""
import os

import numpy as np
import pytest
import torch

import icemix_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (0, 2, 63, 64, 65, 131, 5000)          # around max_pulses = 64; 5000 is above the 4096-pulse LDS limit of the sorts


@pytest.fixture(autouse=True)
def ice_table_from_fixture(monkeypatch):
    monkeypatch.setenv("GRAPHNET_AMD_ICE_TABLE", os.path.join(GOLDEN, "ice_transparency.npz"))


@pytest.fixture(scope="module")
def table():
    return R.load_table()


@pytest.fixture(scope="module")
def batches():
    """F -> (x fp32 [N, F], ptr); the depth is column 2, the flag column F - 1."""
    return {F: R.shapes_batch(F, np.random.default_rng(100 + F), SIZES) for F in (6, 7)}


def _device(x, ptr, L, hlc_col, z_col, table, seed=0, event_ids=None, key_bits=32, **kw):
    from graphnet_amd import ops
    xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    tt = None if z_col < 0 else torch.from_numpy(table).to(DEV)
    ev = None if event_ids is None else torch.as_tensor(np.asarray(event_ids, dtype=np.int64))
    nodes, node_ptr, ids = ops.icemix_nodes(xt, torch.as_tensor(np.asarray(ptr), dtype=torch.int32).to(DEV), L, hlc_col, z_col,
                                            tt, seed, ev, key_bits, **kw)
    return nodes, node_ptr.cpu().numpy(), ids.cpu().numpy()


def _check(x, ptr, L, hlc_col, z_col, table, **kw):
    exp, exp_ptr, exp_ids = R.nodes_batch(x, ptr, L, hlc_col, z_col, table, **kw)
    nodes, node_ptr, ids = _device(x, ptr, L, hlc_col, z_col, table, **kw)
    assert np.array_equal(node_ptr, exp_ptr) and np.array_equal(ids, exp_ids)
    assert nodes.shape == exp.shape and R.same(nodes.cpu().numpy(), exp)
    return exp, exp_ptr, exp_ids


@pytest.mark.parametrize("key_bits", [32, 4])
@pytest.mark.parametrize("ice", [True, False])
@pytest.mark.parametrize("hlc", [True, False])
@pytest.mark.parametrize("F", [6, 7])
def test_shapes_batch_equals_the_restatement(batches, table, F, hlc, ice, key_bits):
    """Events of 0, 2, 63, 64, 65, 131 and 5000 pulses at max_pulses = 64.  key_bits = 4 leaves 16 distinct keys, so the
    threshold key is shared by many pulses and the lowest indices among them are kept."""
    x, ptr = batches[F]
    exp, exp_ptr, exp_ids = _check(x, ptr, 64, F - 1 if hlc else -1, 2 if ice else -1, table, seed=77, key_bits=key_bits)
    # what the restatement alone says about this input
    assert np.diff(exp_ptr).tolist() == [0, 2, 63, 64, 64, 64, 64] and exp.shape[1] == F + 2 * ice
    if hlc:
        flipped = exp[:, F - 1]
        assert set(np.unique(flipped).tolist()) == {0.0, 1.0} and np.isnan(x[exp_ids, F - 1]).any()
        assert np.array_equal(flipped == 1.0, x[exp_ids, F - 1] == 0)
    if ice:
        assert not np.isnan(exp[:, F:]).any()
    if key_bits == 4:
        h = R.keys(77, 6, 5000, 4)
        last = exp_ids[exp_ptr[6]:] - ptr[6]
        t = h[last].max()
        assert (h == t).sum() > (h[last] == t).sum() > 0           # the threshold key: some kept, some not
        assert np.flatnonzero(h == t)[:(h[last] == t).sum()].tolist() == last[h[last] == t].tolist()


def test_max_pulses_one_and_a_large_cap(batches, table):
    x, ptr = batches[7]
    exp, exp_ptr, _ = _check(x, ptr, 1, 6, 2, table, seed=3)
    assert np.diff(exp_ptr).tolist() == [0, 1, 1, 1, 1, 1, 1]
    exp, exp_ptr, exp_ids = _check(x, ptr, 4999, 6, 2, table, seed=3)       # one pulse of the last event dropped
    assert np.diff(exp_ptr).tolist() == [0, 2, 63, 64, 65, 131, 4999]
    exp, exp_ptr, exp_ids = _check(x, ptr, 768, 6, 2, table, seed=3)        # production: the large event alone is cut
    assert np.diff(exp_ptr).tolist() == [0, 2, 63, 64, 65, 131, 768]


def test_depth_outside_the_table_or_nan_gives_nan_in_both_ice_columns(batches, table):
    x, ptr = batches[7]
    x = x.copy()
    lo, hi = np.float32(table[0, 0]), np.float32(table[0, -1])
    below = lo if float(lo) < table[0, 0] else np.nextafter(lo, np.float32(-np.inf))
    above = hi if float(hi) > table[0, -1] else np.nextafter(hi, np.float32(np.inf))
    x[0:300:4, 2] = np.resize(np.asarray([below, above, np.nan, np.inf, -np.inf, -5.0], dtype=np.float32), 75)
    exp, _, exp_ids = _check(x, ptr, 64, 6, 2, table, seed=9)
    bad = ~((x[exp_ids, 2].astype(np.float64) >= table[0, 0]) & (x[exp_ids, 2].astype(np.float64) <= table[0, -1]))
    assert 20 < bad.sum() < len(bad)
    assert np.isnan(exp[bad, 7:]).all() and not np.isnan(exp[~bad, 7:]).any()
    assert R.same(exp[:, :6], x[exp_ids, :6])                      # the rest of the row is exact


def test_two_launches_agree_and_event_ids_name_the_streams(batches, table):
    x, ptr = batches[7]
    a = _device(x, ptr, 64, 6, 2, table, seed=21)
    b = _device(x, ptr, 64, 6, 2, table, seed=21)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and np.array_equal(a[2], b[2])
    c = _device(x, ptr, 64, 6, 2, table, seed=22)
    assert not np.array_equal(a[2], c[2]) and np.array_equal(a[1], c[1])
    ev = [7, 0xFFFFFFFF, 2 ** 31, 3, 12345, 9, 6]
    _, _, ids = _check(x, ptr, 64, 6, 2, table, seed=21, event_ids=ev)
    assert np.array_equal(ids[-64:], a[2][-64:]) and not np.array_equal(ids[-128:-64], a[2][-128:-64])    # event 6 keeps id 6


def test_strided_input_output_pitch_and_empty_batches(batches, table):
    x, ptr = batches[6]
    wide = torch.full((len(x), 11), float("nan"), device=DEV)
    wide[:, 3:9] = torch.from_numpy(x).to(DEV)
    exp, exp_ptr, exp_ids = R.nodes_batch(x, ptr, 64, 5, 2, table, seed=4)
    nodes, node_ptr, ids = _device(wide[:, 3:9], ptr, 64, 5, 2, table, seed=4, out_pitch=12)
    assert nodes.shape == exp.shape and nodes.stride(0) == 12
    assert R.same(nodes.cpu().numpy(), exp) and np.array_equal(node_ptr, exp_ptr) and np.array_equal(ids, exp_ids)
    nodes, node_ptr, ids = _device(torch.zeros((0, 6), device=DEV), [0, 0, 0], 64, 5, 2, table)
    assert nodes.shape == (0, 8) and node_ptr.tolist() == [0, 0, 0] and ids.shape == (0,)
    nodes, node_ptr, ids = _device(torch.zeros((0, 6), device=DEV), [0], 64, 5, -1, table)
    assert nodes.shape == (0, 6) and node_ptr.tolist() == [0]


def _kaggle_events(sizes, seed=8):
    from graphnet_amd.synthetic import icecube86_geometry
    rng = np.random.default_rng(seed)
    geo = icecube86_geometry()
    events = []
    for n in sizes:
        raw = np.empty((n, 6), dtype=np.float64)
        raw[:, :3] = geo[rng.integers(0, len(geo), n), :3]
        raw[:, 3] = rng.uniform(9000, 15000, n)
        raw[:, 4] = rng.uniform(0.2, 30, n)
        raw[:, 5] = rng.integers(0, 2, n)
        events.append(raw)
    return events


NAMES = ["x", "y", "z", "time", "charge", "auxiliary"]


def _graph_definition(node_definition=None):
    import graphnet_amd as g
    nd = node_definition or g.IceMixNodes(input_feature_names=NAMES, max_pulses=64, z_name="z", hlc_name="auxiliary")
    return g.KNNGraph(g.IceCubeKaggle(), node_definition=nd, input_feature_names=NAMES)


def test_batch_from_raw_on_the_device_equals_the_host_path():
    import graphnet_amd as g
    events = _kaggle_events([30, 1, 64, 65, 200, 0, 700])         # the events of 1 and 0 pulses are dropped
    gd = _graph_definition()
    torch.manual_seed(17)
    b = gd.batch_from_raw(events, NAMES, device=DEV)
    torch.manual_seed(17)
    h = gd.batch_from_raw(events, NAMES, device="cpu")
    assert b.x.is_cuda and b.pulse_ids.is_cuda and tuple(b.x.shape) == (30 + 64 * 4, 8)
    # charge = log10(q) / 3: the device's log10f and the host libm's may differ in the last bit (the bound of
    # test_standardize_on_device_matches_oracle); nothing after the standardisation touches the column
    rest = [0, 1, 2, 3, 5, 6, 7]
    assert torch.equal(b.x.cpu()[:, rest].view(torch.int32), h.x[:, rest].view(torch.int32))
    assert torch.allclose(b.x.cpu()[:, 4], h.x[:, 4], rtol=2e-6, atol=1e-7)
    # ... and the host path on the pulses as the device standardised them gives the device's rows, charge included
    plain = _graph_definition(g.NodesAsPulses()).batch_from_raw(events, NAMES, device=DEV)
    torch.manual_seed(17)
    again = gd._node_definition.sample_batch(plain.x.cpu(), plain.ptr.cpu().to(torch.int32))
    assert torch.equal(again[0].view(torch.int32), b.x.cpu().view(torch.int32)) and torch.equal(again[2], b.pulse_ids.cpu())
    assert torch.equal(b.ptr.cpu(), h.ptr) and b.ptr.tolist() == [0, 30, 94, 158, 222, 286]
    assert torch.equal(b.batch.cpu(), h.batch) and torch.equal(b.pulse_ids.cpu(), h.pulse_ids)
    assert b.n_pulses.tolist() == h.n_pulses.tolist() == [30, 64, 65, 200, 700]
    torch.manual_seed(18)
    assert not torch.equal(gd.batch_from_raw(events, NAMES, device=DEV).pulse_ids, b.pulse_ids)
    # the stand-alone call on one event, on the device
    nd = gd._node_definition
    one = torch.from_numpy(np.ascontiguousarray(h.x[:30, :6].numpy())).to(DEV)
    one[:, 5] = 1.0 - one[:, 5]                                   # undo the flip: the raw flags
    assert torch.equal(nd(one)[0].x.cpu().view(torch.int32), h.x[:30].view(torch.int32))


def test_deepice_on_the_icemix_batch():
    """A small DeepIce on the IceMixNodes batch against the same model on a NodesAsPulses batch of ``x[pulse_ids]`` with the
    flag flipped: the inputs are bit-equal, so the outputs agree within the 1e-5 of "an event alone and inside the batch"."""
    import graphnet_amd as g
    from test_gpu_tito import rel_err
    events = _kaggle_events([30, 64, 65, 200, 700], seed=9)
    torch.manual_seed(23)
    b = _graph_definition().batch_from_raw(events, NAMES, device=DEV)
    plain = _graph_definition(g.NodesAsPulses()).batch_from_raw(events, NAMES, device=DEV)
    picked = plain.x[b.pulse_ids.long()].clone()
    picked[:, 5] = (picked[:, 5] == 0).float()
    assert torch.equal(picked, b.x[:, :6])
    p = g.Batch(x=picked)
    p.ptr, p.batch, p.n_pulses = b.ptr.clone(), b.batch.clone(), b.n_pulses.clone()
    torch.manual_seed(1)
    m = g.DeepIce(hidden_dim=64, head_size=32, seq_length=32, depth=2, depth_rel=2, n_rel=1).to(DEV).set_backend(dtype="fp32")
    y = m(b)
    with torch.no_grad():
        yp = m(p)
    err = rel_err(y.detach(), yp)
    print(f"DeepIce on the IceMixNodes batch vs the picked pulses: {err:.3e}")
    assert y.shape == (5, 64) and err < 1e-5
    (y ** 2).mean().backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
