"""CPU: ``IceMixNodes`` - constructor surface, the ice table against what the reference's ``ice_transparency`` returned
(``golden/icemix_nodes_expected.npz``), the host path of the ``gn_icemix_nodes`` contract on the bundled events, and the
uniformity of the contract's sampler."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import icemix_reference as R
from graphnet_amd import IceMixNodes, ModelConfig
from graphnet_amd.graphs import ice_interp_host, ice_table_host, icemix_keys, icemix_nodes_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLE_NPZ = os.path.join(GOLDEN, "ice_transparency.npz")


@pytest.fixture(autouse=True)
def ice_table_from_fixture(monkeypatch):
    monkeypatch.setenv("GRAPHNET_AMD_ICE_TABLE", TABLE_NPZ)


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(GOLDEN, "icemix_nodes_expected.npz"))


@pytest.fixture(scope="module")
def events():
    """name -> (fp32 [N, F] with the z column divided by 600 so that every pulse lies inside the ice table, ptr)."""
    ev = np.load(os.path.join(GOLDEN, "reference_events.npz"))
    out = {}
    for name in ("upgrade", "prometheus"):
        x = ev[name + "_x"].astype(np.float32)
        x[:, 2] = x[:, 2] / np.float32(600.0)
        out[name] = (x, ev[name + "_ptr"].astype(np.int32))
    return out


# ---- constructor surface ---------------------------------------------------------------------------------------------
def test_constructor_surface_is_the_references():
    params = inspect.signature(IceMixNodes.__init__).parameters
    assert list(params) == ["self", "input_feature_names", "max_pulses", "z_name", "hlc_name", "add_ice_properties", "ice_args"]
    assert [params[k].default for k in list(params)[1:]] == [None, 768, "dom_z", "hlc", True, {"z_offset": None, "z_scaling": None}]
    nd = IceMixNodes()
    names = ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "hlc", "rde"]
    assert nd.input_feature_names == names and nd.all_features == names + ["scatt_lenght", "abs_lenght"]
    assert nd.n_features == nd.nb_outputs == 9 and nd.max_length == 768
    assert nd.z_name == "dom_z" and nd.hlc_name == "hlc" and nd.add_ice_properties is True
    assert nd.feature_indexes == {n: i for i, n in enumerate(names)}
    bare = IceMixNodes(input_feature_names=["a", "hlc"], max_pulses=5, add_ice_properties=False)
    assert bare.all_features == ["a", "hlc"] and bare.n_features == bare.nb_outputs == 2 and bare.max_length == 5


def test_missing_z_raises_and_missing_hlc_warns():
    with pytest.raises(ValueError, match="z name 'dom_z' not found in input_feature_names"):
        IceMixNodes(input_feature_names=["x", "y", "z"])
    with pytest.warns(UserWarning, match="hlc name 'hlc' not found.*subsampling will be random"):
        nd = IceMixNodes(input_feature_names=["x", "y", "z"], z_name="z")
    assert nd.hlc_name is None and nd.all_features == ["x", "y", "z", "scatt_lenght", "abs_lenght"]


def test_without_a_table_construction_names_the_three_ways(monkeypatch, expected):
    monkeypatch.delenv("GRAPHNET_AMD_ICE_TABLE")
    monkeypatch.setattr(IceMixNodes, "ice_table", None)
    monkeypatch.setitem(sys.modules, "graphnet", None)             # not importable, wherever this runs
    monkeypatch.setitem(sys.modules, "graphnet.constants", None)
    with pytest.raises(RuntimeError) as err:
        IceMixNodes()
    for way in ("GRAPHNET_AMD_ICE_TABLE", "ice_table = (depth, scattering_len, absorption_len)", "graphnet"):
        assert way in str(err.value)
    IceMixNodes(add_ice_properties=False)                          # needs no table
    raw = np.load(TABLE_NPZ)
    monkeypatch.setattr(IceMixNodes, "ice_table", tuple(raw[k] for k in ("depth", "scattering_len", "absorption_len")))
    nd = IceMixNodes()                                             # assigned on the class
    assert np.array_equal(nd._table(), R.load_table())
    nd.ice_table = (raw["depth"], raw["scattering_len"] * 2.0 + 1.0, raw["absorption_len"])      # replaced on the instance
    assert np.array_equal(nd._table()[2], R.load_table()[2]) and np.array_equal(nd._table()[0], R.load_table()[0])
    assert np.abs(nd._table()[1] - R.load_table()[1]).max() < 1e-12          # the robust scaler undoes an affine map


def test_model_config_round_trip(tmp_path):
    nd = IceMixNodes(input_feature_names=["x", "y", "z", "time", "charge", "auxiliary"], max_pulses=192, z_name="z",
                     hlc_name="auxiliary", ice_args={"z_offset": -1900.0, "z_scaling": 450.0})
    nd.save_config(str(tmp_path / "nodes.yml"))
    back = IceMixNodes.from_config(str(tmp_path / "nodes.yml"))
    assert isinstance(back, IceMixNodes) and back.amd_config.as_dict() == nd.amd_config.as_dict()
    assert back.max_length == 192 and back.hlc_name == "auxiliary" and back.n_features == 8
    assert np.array_equal(back._table(), R.load_table("o_"))
    again = ModelConfig("IceMixNodes", nd.amd_config.as_dict()["arguments"]).construct()
    assert again.all_features == nd.all_features


# ---- the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["d_", "o_"])
def test_table_and_functions_equal_the_references_bit_for_bit(expected, tag):
    raw = np.load(TABLE_NPZ)
    z_offset, z_scaling = (None if np.isnan(v) else float(v) for v in expected[tag + "ice_args"])
    table = ice_table_host(raw["depth"], raw["scattering_len"], raw["absorption_len"], z_offset, z_scaling)
    assert table.dtype == np.float64 and table.shape == (3, 110)
    for row, name in zip(table, ("z_norm", "scatt", "abs")):
        assert np.array_equal(row, expected[tag + name]), name    # numpy scaler == RobustScaler, fp64
    z = expected[tag + "z"]
    assert z.dtype == np.float32 and len(z) > 9000
    fs, fa = ice_interp_host(table, z)
    assert fs.dtype == np.float64
    assert R.same(fs.astype(np.float32), expected[tag + "fs32"]) and R.same(fa.astype(np.float32), expected[tag + "fa32"])
    # the one-pulse restatement of the header says the same
    pick = np.r_[0:len(z):37, len(z) - 400:len(z)]
    one = np.asarray([R.ice(table, v) for v in z[pick]], dtype=np.float32)
    assert R.same(one[:, 0], expected[tag + "fs32"][pick]) and R.same(one[:, 1], expected[tag + "fa32"][pick])


def test_depth_outside_the_table_or_nan_raises_on_the_host():
    table = R.load_table()
    lo, hi = np.float32(table[0, 0]), np.float32(table[0, -1])
    below = lo if float(lo) < table[0, 0] else np.nextafter(lo, np.float32(-np.inf))
    above = hi if float(hi) > table[0, -1] else np.nextafter(hi, np.float32(np.inf))
    for bad in (below, above, np.float32(np.nan), np.float32(np.inf)):
        with pytest.raises(ValueError, match="outside the interpolation range"):
            ice_interp_host(table, np.asarray([0.0, bad], dtype=np.float32))
        assert np.isnan(R.ice(table, bad)).all()
    nd = IceMixNodes(max_pulses=4)
    x = torch.zeros(3, 7)
    x[1, 2] = 1.2                                                  # 600 m above the detector centre: no ice data there
    with pytest.raises(ValueError, match="outside the interpolation range"):
        nd(x)
    with pytest.raises(ValueError):
        nd.f_scattering(np.float32(-1.2))
    assert np.float32(nd.f_absoprtion(np.float32(0.25))) == R.ice(table, 0.25)[1]


# ---- the host path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", [("upgrade", 64), ("prometheus", 128)])
def test_host_path_on_bundled_events(events, name, L):
    x, ptr = events[name]
    F = x.shape[1]
    names = ["dom_x", "dom_y", "dom_z"] + [f"f{i}" for i in range(3, F - 1)] + ["hlc"]
    x = x.copy()
    x[::3, F - 1] = 0.0                                            # a flag column with zeros and other values
    nd = IceMixNodes(input_feature_names=names, max_pulses=L)
    nodes, node_ptr, ids = (t.numpy() for t in nd.sample_batch(torch.from_numpy(x), torch.from_numpy(ptr), seed=11))
    n = np.diff(ptr)
    if name == "upgrade":
        assert n.tolist() == [145, 94, 85, 167, 134]               # every event above max_pulses
    assert np.array_equal(np.diff(node_ptr), np.minimum(n, L)) and nodes.shape == (node_ptr[-1], F + 2)
    assert nodes.dtype == np.float32 and ids.dtype == np.int32 and node_ptr.dtype == np.int32
    for b in range(len(n)):
        mine = ids[node_ptr[b]:node_ptr[b + 1]]
        assert (np.diff(mine) > 0).all() and (len(mine) == 0 or (mine[0] >= ptr[b] and mine[-1] < ptr[b + 1]))
        if n[b] <= L:
            assert np.array_equal(mine, np.arange(ptr[b], ptr[b + 1]))
    assert R.same(nodes[:, :F - 1], x[ids, :F - 1])
    assert np.array_equal(nodes[:, F - 1], (x[ids, F - 1] == 0).astype(np.float32)) and 0 < nodes[:, F - 1].sum() < len(nodes)
    exp = R.nodes_batch(x, ptr, L, F - 1, 2, R.load_table(), 11)
    assert R.same(nodes, exp[0]) and np.array_equal(node_ptr, exp[1]) and np.array_equal(ids, exp[2])
    # the same ids whatever the hlc column holds, and without one
    y = x.copy()
    y[:, F - 1] = 1.0 - y[:, F - 1]
    assert np.array_equal(nd.sample_batch(torch.from_numpy(y), torch.from_numpy(ptr), seed=11)[2].numpy(), ids)
    with pytest.warns(UserWarning):
        no_hlc = IceMixNodes(input_feature_names=names, max_pulses=L, hlc_name=None)
    plain, _, ids2 = no_hlc.sample_batch(torch.from_numpy(x), torch.from_numpy(ptr), seed=11)
    assert np.array_equal(ids2.numpy(), ids) and R.same(plain.numpy()[:, F - 1], x[ids, F - 1])


def test_shorter_and_equal_events_are_the_identity_with_the_flip(events):
    x, _ = events["upgrade"]
    x = x[:64, :7].copy()
    x[::2, 5] = 0.0
    nd = IceMixNodes(max_pulses=64)
    for n in (1, 63, 64):
        out = nd(torch.from_numpy(x[:n].copy()))[0].x.numpy()
        assert out.shape == (n, 9) and R.same(out[:, [0, 1, 2, 3, 4, 6]], x[:n, [0, 1, 2, 3, 4, 6]])
        assert np.array_equal(out[:, 5], (x[:n, 5] == 0).astype(np.float32))
        assert R.same(out, R.nodes_batch(x[:n], [0, n], 64, 5, 2, R.load_table())[0])
    names = nd(torch.from_numpy(x[:3].copy()))[1]
    assert names == nd.all_features


def test_seeds_and_event_ids(events):
    x, ptr = events["upgrade"]
    xt, pt = torch.from_numpy(x[:, :7].copy()), torch.from_numpy(ptr)
    nd = IceMixNodes(max_pulses=64)
    a, b, c = (nd.sample_batch(xt, pt, seed=s)[2] for s in (5, 5, 6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    ev = nd.sample_batch(xt, pt, seed=5, event_ids=[4, 3, 2, 1, 0])[2]
    assert not torch.equal(ev, a)
    exp = R.nodes_batch(x[:, :7], ptr, 64, 5, 2, R.load_table(), 5, [4, 3, 2, 1, 0])
    assert np.array_equal(ev.numpy(), exp[2])
    # event 2 under id 2 is event 2 of the default ordinals
    assert torch.equal(ev[128:192], a[128:192])
    # seed=None: torch's global generator
    torch.manual_seed(3)
    d, e = nd.sample_batch(xt, pt)[2], nd.sample_batch(xt, pt)[2]
    torch.manual_seed(3)
    f = nd.sample_batch(xt, pt)[2]
    assert torch.equal(d, f) and not torch.equal(d, e)
    # uint32 wrap-around of seed and ids, the package's keys against the restatement's
    for seed, e_id, bits in ((0xFFFFFFFF, 0xFFFFFFFE, 32), (7, 123456789, 4), (2 ** 31, 2 ** 31, 17)):
        assert np.array_equal(icemix_keys(seed, e_id, 300, bits), R.keys(seed, e_id, 300, bits))
    few = R.keys(7, 123456789, 300, 4)
    assert few.max() < 16 and len(np.unique(few)) == 16
    tie = icemix_nodes_host(x[:145, :7], [0, 145], 64, seed=7, event_ids=[9], key_bits=4)[2]
    assert tie.tolist() == R.kept(7, 9, 145, 64, 4)


# ---- uniformity of the contract's sampler ----------------------------------------------------------------------------
def _z_scores(mask, n, L):
    draws = len(mask)
    p = L / n
    z = (mask.sum(0) - draws * p) / np.sqrt(draws * p * (1 - p))
    p2 = L * (L - 1) / (n * (n - 1))
    pair = ((mask[:, 0] & mask[:, 1]).sum() - draws * p2) / np.sqrt(draws * p2 * (1 - p2))
    return float(np.abs(z).max()), float(pair)


@pytest.mark.parametrize("n,L,draws", [(24, 8, 6000), (65, 64, 4000), (300, 192, 2000)])
def test_every_pulse_is_kept_equally_often(n, L, draws):
    """Per-pulse inclusion against the binomial, and pulses 0 and 1 kept together, over seeds 1234 + s with event id 7.
    A condition on the hash: largest |z| 2.52 / 2.50 / 2.93, pair z -1.31 / 0.56 / -0.85."""
    mask = R.kept_many(1234 + np.arange(draws), 7, n, L)
    assert (mask.sum(1) == L).all()
    worst, pair = _z_scores(mask, n, L)
    print(f"n={n} L={L} draws={draws}: largest |z| {worst:.2f}, pair z {pair:.2f}")
    assert worst < 5 and abs(pair) < 5
    # the package's host path draws the same subsets
    for s in (0, draws - 1):
        ids = icemix_nodes_host(np.zeros((n, 1), np.float32), [0, n], L, seed=1234 + s, event_ids=[7])[2]
        assert np.array_equal(np.flatnonzero(mask[s]), ids)


def test_event_ids_are_independent_streams():
    """Seed 99, event ids 0..5999 at (24, 8): largest |z| 1.92."""
    mask = R.kept_many(99, np.arange(6000), 24, 8)
    worst, pair = _z_scores(mask, 24, 8)
    print(f"by event id: largest |z| {worst:.2f}, pair z {pair:.2f}")
    assert worst < 5 and abs(pair) < 5


# ---- GraphDefinition -------------------------------------------------------------------------------------------------
def test_graph_definition_forward_per_event():
    import graphnet_amd as g
    from graphnet_amd.synthetic import icecube86_geometry
    names = ["x", "y", "z", "time", "charge", "auxiliary"]
    gd = g.KNNGraph(g.IceCubeKaggle(), node_definition=IceMixNodes(input_feature_names=names, max_pulses=64, z_name="z",
                                                                   hlc_name="auxiliary"), input_feature_names=names)
    assert gd.nb_outputs == 8 and gd.output_feature_names == names + ["scatt_lenght", "abs_lenght"]
    rng = np.random.default_rng(2)
    geo = icecube86_geometry()
    for n in (40, 64, 100):
        raw = np.empty((n, 6), dtype=np.float64)
        raw[:, :3] = geo[rng.integers(0, len(geo), n), :3]
        raw[:, 3] = rng.uniform(9000, 15000, n)
        raw[:, 4] = rng.uniform(0.2, 30, n)
        raw[:, 5] = rng.integers(0, 2, n)
        torch.manual_seed(n)
        data = gd(raw.copy(), names)
        assert tuple(data.x.shape) == (min(n, 64), 8) and int(data.n_pulses) == n
        assert data.features == names + ["scatt_lenght", "abs_lenght"] and torch.equal(data.abs_lenght, data.x[:, 7])
        assert not torch.isnan(data.x).any()
        # rows are pulses of the event in their order, auxiliary flipped
        std = g.IceCubeKaggle()(torch.tensor(raw, dtype=torch.float32), names).numpy()
        rows = [int(np.flatnonzero((std[:, :5] == r[:5]).all(1))[0]) for r in data.x.numpy()]
        assert rows == sorted(rows) and len(set(rows)) == len(rows)
        assert np.array_equal(data.x[:, 5].numpy(), (std[rows, 5] == 0).astype(np.float32))
