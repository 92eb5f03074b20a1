"""CPU: the ``PercentileClusters`` contract.  The loop-per-cluster restatement (``percentile_reference.py``) equals what
the reference's ``cluster_summarize_with_percentiles`` recorded (``golden/percentile_clusters_expected.npz``), the
product's vectorised host path equals the restatement, and the class behaves as the reference's inside a
``GraphDefinition``.  The device path is compared against the same restatement in tests/test_gpu_percentile.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import graphnet_amd as g
import percentile_reference as R
from graphnet_amd.graphs import percentile_clusters_host
from graphnet_amd.synthetic import FEATURES_ICECUBE86

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PCT = [0, 10, 50, 90, 100]
XYZ = ["dom_x", "dom_y", "dom_z"]


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "percentile_clusters_expected.npz")), np.load(os.path.join(GOLDEN, "reference_events.npz"))


def _fixture_events(recorded, name):
    fx, ev = recorded
    x, ptr = ev[name + "_x"].astype(np.float32), ev[name + "_ptr"]
    nb = len(fx[name + "_node_ptr"]) - 1
    return x[:ptr[nb]], ptr[:nb + 1], fx[name + "_percentiles"].tolist(), fx[name + "_nodes"], fx[name + "_node_ptr"]


def _host_batch(x, ptr, cl, sm, pct, add_counts=True):
    parts = [percentile_clusters_host(x[lo:hi], cl, sm, pct, add_counts) for lo, hi in zip(ptr[:-1], ptr[1:])]
    return np.concatenate(parts, axis=0)


# ------------------------------------------------------------------------------ 1. restatement == the reference's results
@pytest.mark.parametrize("name,events,clusters", [("prometheus", 50, 1511), ("deepcore", 5, 38), ("upgrade", 2, 154)])
def test_restatement_equals_the_recorded_reference_results(recorded, name, events, clusters):
    x, ptr, pct, nodes, node_ptr = _fixture_events(recorded, name)
    assert len(ptr) - 1 == events and len(nodes) == clusters and nodes.dtype == np.float32
    assert pct == ([0, 50, 100] if name == "upgrade" else PCT)
    got, got_ptr = R.cluster_batch(x, ptr, [0, 1, 2], list(range(3, x.shape[1])), pct)
    assert np.array_equal(got_ptr, node_ptr)
    assert R.same(got, nodes)                                   # entry for entry, row order and counts included


# ------------------------------------------------------------------------------ 2. the reference's own check
def test_percentiles_of_every_dom_match_a_pandas_group_by(recorded):
    import pandas as pd
    x, ptr, pct, _, _ = _fixture_events(recorded, "prometheus")
    names = ["sensor_pos_x", "sensor_pos_y", "sensor_pos_z", "t"]
    ev = x[ptr[0]:ptr[1]]
    nd = g.PercentileClusters(names[:3], pct, add_counts=False, input_feature_names=names)
    nodes, out_names = nd(torch.from_numpy(ev))
    assert out_names == names[:3] + [f"t_pct{p}" for p in pct]
    got = pd.DataFrame(nodes.x.numpy(), columns=out_names)
    groups = pd.DataFrame(ev.astype(np.float64), columns=names).groupby(names[:3])["t"]
    assert len(got) == groups.ngroups
    for _, row in got.iterrows():
        times = groups.get_group(tuple(float(row[n]) for n in names[:3])).to_numpy()
        for p in pct:
            assert np.isclose(row[f"t_pct{p}"], np.percentile(times, p))


# ------------------------------------------------------------------------------ 3. product host path == restatement
def test_host_path_equals_restatement_on_the_recorded_events(recorded):
    for name in ("prometheus", "deepcore", "upgrade"):
        x, ptr, pct, nodes, _ = _fixture_events(recorded, name)
        assert R.same(_host_batch(x, ptr, [0, 1, 2], list(range(3, x.shape[1])), pct), nodes)


def test_host_path_equals_restatement_on_the_generated_batch():
    x, ptr = R.shapes_batch()
    exp, exp_ptr = R.cluster_batch(x, ptr, [0, 1, 2], [3, 4, 5], PCT)
    assert np.diff(exp_ptr).tolist() == [1, 1, 1, 2, 15, 16, 15, 62, 64, 148, 270, 503]
    assert R.same(_host_batch(x, ptr, [0, 1, 2], [3, 4, 5], PCT), exp)


@pytest.mark.parametrize("cluster_nan", [False, True])
@pytest.mark.parametrize("add_counts", [True, False])
@pytest.mark.parametrize("cl", [[0, 1, 2], [4, 0, 2], [2, 0], [1]])
def test_host_path_equals_restatement_on_ties_and_specials(cl, add_counts, cluster_nan):
    x = R.grid_event(cluster_nan)
    sm = [c for c in range(6) if c not in cl]
    exp, members = R.cluster_event(x, cl, sm, PCT, add_counts)
    got = percentile_clusters_host(x, cl, sm, PCT, add_counts)
    assert got.dtype == np.float32 and R.same(got, exp)
    assert sum(len(m) for m in members) == len(x) and all(m == sorted(m) for m in members)
    if cl == [0, 1, 2]:
        assert max(len(m) for m in members) >= 40               # the forty coincident pulses
        assert np.isnan(exp[:, 3:18]).any() and np.isinf(exp[:, 3:18]).any()
        zeros = x[x[:, 0] == 0, 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()
        # -0.0 clusters with +0.0: as many clusters as distinct positions under ==
        if not cluster_nan:
            assert len(exp) == len(np.unique(x[:, :3] + np.float32(0.0), axis=0))
        else:
            assert np.isnan(exp[-1, 2]) and len(members[-1]) == 3 and not np.isnan(exp[:-1, :3]).any()


# ------------------------------------------------------------------------------ 4. inside a GraphDefinition
def _deepcore_event(recorded):
    _, ev = recorded
    ptr = ev["deepcore_ptr"]
    i = int(np.argmax(np.diff(ptr)))
    return ev["deepcore_x"][ptr[i]:ptr[i + 1]].copy()


def test_graph_definition_with_percentile_clusters(recorded):
    raw = _deepcore_event(recorded)
    nd = g.PercentileClusters(XYZ, [0, 50, 100])
    gd = g.GraphDefinition(g.IceCube86(), node_definition=nd, input_feature_names=FEATURES_ICECUBE86)
    summarised = [f for f in FEATURES_ICECUBE86 if f not in XYZ]
    names = XYZ + [f"{f}_pct{p}" for f in summarised for p in [0, 50, 100]] + ["counts"]
    assert gd.output_feature_names == names and gd.nb_outputs == nd.nb_outputs == len(names) == 16
    assert gd.nb_inputs == nd.nb_inputs == 7
    out = gd(raw.copy(), FEATURES_ICECUBE86)
    pulses = g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86)(raw.copy(), FEATURES_ICECUBE86)
    exp, _ = R.cluster_event(pulses.x.numpy(), [0, 1, 2], [3, 4, 5, 6], [0, 50, 100])
    assert out.x.dtype == torch.float32 and R.same(out.x.numpy(), exp)
    assert int(out.n_pulses) == len(raw) and out.x.shape[0] == len(exp) < len(raw)
    assert out["features"] == names
    for i, name in enumerate(names):
        assert torch.equal(out[name], out.x[:, i])
    srt = g.GraphDefinition(g.IceCube86(), node_definition=g.PercentileClusters(XYZ, [0, 50, 100]),
                            input_feature_names=FEATURES_ICECUBE86, sort_by="dom_y")
    out_s = srt(raw.copy(), FEATURES_ICECUBE86)
    assert out_s.x.shape == out.x.shape and bool((out_s.x[1:, 1] >= out_s.x[:-1, 1]).all())
    assert not torch.equal(out_s.x, out.x)
    assert torch.equal(out_s.x, out.x[out.x[:, 1].sort()[1]])


def test_inactive_sensors_and_string_mask_on_clustered_nodes():
    """The reference's three inequalities (``tests/models/test_graph_definition.py:157-163``) on the packaged IceCube-86
    table, with the feature columns that the table can pad."""
    import pandas as pd
    d = np.load(os.path.join(os.path.dirname(g.__file__), "geometry_tables", "icecube86.npz"))
    names = ["dom_x", "dom_y", "dom_z", "rde", "pmt_area"]
    table = pd.DataFrame(d["table"], columns=names)
    table["string"] = d["string"].astype(np.int64)
    table["sensor_id"] = np.arange(len(table), dtype=np.int64)
    ids = np.array([10, 11, 11, 500, 2000, 2000, 2000, 4000, 5406])
    raw = table.iloc[ids][names].to_numpy(dtype=np.float64)
    strings = sorted(set(table["string"].tolist()))[:50]

    def build(**kw):
        det = g.IceCube86()
        det.geometry_table = table
        nd = g.PercentileClusters(XYZ, [0, 50, 100], input_feature_names=names)
        return g.GraphDefinition(det, node_definition=nd, input_feature_names=names, **kw)(raw.copy(), names)

    original = build()
    inactive = build(add_inactive_sensors=True)
    masked = build(add_inactive_sensors=True, string_mask=strings)
    assert original.x.shape[0] == len(set(ids.tolist())) and inactive.x.shape[0] == len(table)
    assert original.x.shape[0] < inactive.x.shape[0]
    assert masked.x.shape[0] < inactive.x.shape[0]
    assert masked.x.shape[0] > original.x.shape[0]


# ------------------------------------------------------------------------------ 5. NodesAsPulses is unchanged
def test_nodes_as_pulses_is_unchanged():
    nd = g.NodesAsPulses()
    with pytest.raises(AttributeError):
        nd(torch.zeros(3, 7))
    nd.set_output_feature_names(FEATURES_ICECUBE86)
    nd.set_number_of_inputs(list(FEATURES_ICECUBE86))
    assert nd._output_feature_names == list(FEATURES_ICECUBE86) and nd.nb_outputs == 7 and nd.nb_inputs == 7
    x = torch.randn(5, 7)
    data, names = nd(x)
    assert data.x is x and names == list(FEATURES_ICECUBE86)
    assert g.NodesAsPulses(input_feature_names=["a", "b"]).nb_outputs == 2
    gd = g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86)
    assert gd.output_feature_names == list(FEATURES_ICECUBE86) and gd.nb_outputs == 7


def test_percentile_clusters_needs_its_feature_names():
    nd = g.PercentileClusters(XYZ, [10, 50, 90])
    with pytest.raises(AttributeError):
        nd(torch.zeros(4, 7))
    nd = g.PercentileClusters(XYZ, [10, 50, 90], add_counts=False, input_feature_names=FEATURES_ICECUBE86)
    assert nd.nb_outputs == 3 + 4 * 3 and nd._output_feature_names[3] == "dom_time_pct10"
    data, _ = nd(torch.zeros(4, 7))
    assert tuple(data.x.shape) == (1, 15) and data.x.dtype == torch.float32


# ------------------------------------------------------------------------------ 6. ModelConfig round trip
def test_model_config_round_trip(tmp_path, recorded):
    gd = g.KNNGraph(g.IceCube86(), node_definition=g.PercentileClusters(XYZ, [10, 50, 90], add_counts=False),
                    input_feature_names=FEATURES_ICECUBE86, nb_nearest_neighbours=6)
    path = str(tmp_path / "graph.yml")
    gd.save_config(path)
    text = open(path).read()
    assert "PercentileClusters" in text and "cluster_on" in text
    again = g.Model.from_config(path)
    assert type(again) is g.KNNGraph and type(again._node_definition) is g.PercentileClusters
    assert again._node_definition._cluster_on == XYZ and again._node_definition._percentiles == [10, 50, 90]
    assert again._node_definition._add_counts is False and again.output_feature_names == gd.output_feature_names
    raw = _deepcore_event(recorded)
    a, b = gd(raw.copy(), FEATURES_ICECUBE86), again(raw.copy(), FEATURES_ICECUBE86)
    assert torch.equal(a.x, b.x) and a.knn_k == b.knn_k == 6
    alone = g.Model.from_config(g.PercentileClusters(XYZ, [50], input_feature_names=FEATURES_ICECUBE86).config)
    assert alone.nb_outputs == 8


def test_batch_from_raw_on_the_cpu_clusters_event_by_event(recorded):
    _, ev = recorded
    ptr = ev["deepcore_ptr"]
    events = [ev["deepcore_x"][ptr[i]:ptr[i + 1]] for i in range(5)]
    gd = g.KNNGraph(g.IceCube86(), node_definition=g.PercentileClusters(XYZ, [10, 50, 90]), input_feature_names=FEATURES_ICECUBE86)
    b = gd.batch_from_raw(events, FEATURES_ICECUBE86, device="cpu")
    per_event = [gd(e.copy(), FEATURES_ICECUBE86) for e in events]
    assert torch.equal(b.x, torch.cat([d.x for d in per_event]))
    assert b.ptr.tolist() == np.cumsum([0] + [d.x.shape[0] for d in per_event]).tolist()
    assert b.n_pulses.tolist() == [len(e) for e in events]
    assert b.batch.tolist() == np.repeat(np.arange(5), [d.x.shape[0] for d in per_event]).tolist()

    class Other(g.graphs.NodeDefinition):
        def _define_output_feature_names(self, names):
            return names

        def _construct_nodes(self, x):
            return g.Data(x=x)

    with pytest.raises(NotImplementedError, match="Other"):
        g.KNNGraph(g.IceCube86(), node_definition=Other(), input_feature_names=FEATURES_ICECUBE86).batch_from_raw(
            events, FEATURES_ICECUBE86, device="cpu")


# ------------------------------------------------------------------------------ 7. the C entry
@pytest.fixture(scope="module")
def lib():
    from graphnet_amd import _lib
    return _lib.lib()


def _call(lib, N=10, B=1, ldx=6, cl=(0, 1, 2), sm=(3, 4, 5), q=(0.1, 0.5, 0.9), add_counts=1, ldo=None, C=None, S=None, P=None,
          null=()):
    """Every device pointer is a dummy address unless named in ``null``: the calls below are all rejected on the host."""
    buf = ctypes.create_string_buffer(64)
    dev = {k: (None if k in null else ctypes.addressof(buf)) for k in ("x", "ptr", "out", "out_ptr", "work")}
    cl_a, sm_a, q_a = (ctypes.c_int32 * 8)(*cl), (ctypes.c_int32 * 32)(*sm), (ctypes.c_double * 16)(*q)
    host = {"cl": ctypes.cast(cl_a, ctypes.c_void_p), "sm": ctypes.cast(sm_a, ctypes.c_void_p), "q": ctypes.cast(q_a, ctypes.c_void_p)}
    for k in null:
        if k in host:
            host[k] = None
    C, S, P = len(cl) if C is None else C, len(sm) if S is None else S, len(q) if P is None else P
    ldo = C + S * P + add_counts if ldo is None else ldo
    rc = lib.gn_percentile_clusters(dev["x"], ldx, N, dev["ptr"], B, host["cl"], C, host["sm"], S, host["q"], P, add_counts,
                                    dev["out"], ldo, dev["out_ptr"], dev["work"], None)
    return rc, lib.gn_last_error()


def test_the_c_entry_is_exported_and_rejects_bad_arguments_on_the_host(lib):
    from graphnet_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "graphnet_amd.h")).read()
    for name in ("gn_percentile_clusters", "gn_percentile_work_ints", "gn_percentile_lds_max"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
    assert lib.gn_abi_version() == 7
    assert lib.gn_percentile_lds_max() >= 1024
    sizes = [lib.gn_percentile_work_ints(4, n) for n in (0, 100, 5000, 100_000)]
    assert sizes[0] >= 4 and all(b > a for a, b in zip(sizes[:-1], sizes[1:])) and sizes[-1] >= 3 * 100_000
    assert lib.gn_percentile_work_ints(4, lib.gn_percentile_lds_max() + 1) > 5 * lib.gn_percentile_lds_max()
    assert lib.gn_percentile_work_ints(-1, 5) == -1 and lib.gn_percentile_work_ints(1, -5) == -1
    bad = [
        (dict(C=0), b"1<=C<=8"), (dict(C=9), b"1<=C<=8"), (dict(S=0), b"1<=S<=32"), (dict(S=33), b"1<=S<=32"),
        (dict(P=0), b"1<=P<=16"), (dict(P=17), b"1<=P<=16"),
        (dict(q=(0.1, -0.01, 0.9)), b"0 <= q <= 1"), (dict(q=(0.1, 1.01, 0.9)), b"0 <= q <= 1"),
        (dict(q=(0.1, float("nan"), 0.9)), b"0 <= q <= 1"),
        (dict(cl=(0, 1, 1)), b"distinct"), (dict(sm=(3, 4, 0)), b"distinct"), (dict(sm=(3, 3, 5)), b"distinct"),
        (dict(cl=(0, 1, 6)), b"out of range"), (dict(sm=(3, 4, -1)), b"out of range"), (dict(ldx=5), b"out of range"),
        (dict(ldo=12), b"ldo"), (dict(add_counts=0, ldo=11), b"ldo"),
        (dict(N=-1), b"N"), (dict(B=-1), b"B"),
        (dict(null=("cl",)), b"cluster_cols_host"), (dict(null=("sm",)), b"summ_cols_host"), (dict(null=("q",)), b"q_host"),
        (dict(null=("x",)), b"need x"), (dict(null=("out",)), b"need x"), (dict(null=("work",)), b"need x"),
        (dict(null=("ptr",)), b"ptr[B+1]"), (dict(null=("out_ptr",)), b"ptr[B+1]"),
    ]
    for kw, what in bad:
        rc, msg = _call(lib, **kw)
        assert rc != 0 and b"gn_percentile_clusters" in msg and what in msg, (kw, rc, msg)
    # nothing to do: no pointer is touched, no launch
    assert lib.gn_percentile_clusters(None, 6, 0, None, 0, *_host_lists(), 3, 1, None, 13, None, None, None) == 0


def _host_lists():
    cl, sm, q = (ctypes.c_int32 * 3)(0, 1, 2), (ctypes.c_int32 * 3)(3, 4, 5), (ctypes.c_double * 3)(0.1, 0.5, 0.9)
    _host_lists.keep = (cl, sm, q)
    return ctypes.cast(cl, ctypes.c_void_p), 3, ctypes.cast(sm, ctypes.c_void_p), 3, ctypes.cast(q, ctypes.c_void_p)
