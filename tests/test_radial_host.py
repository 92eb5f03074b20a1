"""CPU: the host side of ``RadialEdges`` - the public class, the C entry's argument validation, the record a CPU ``Data``
carries to the backbone, the config round trip, and the pin of the tests' numpy reference (no device ops)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import graphnet_amd as g
from graphnet_amd.data import select_events
from graphnet_amd.graphs import RADIAL_RECORD, radial_record
from graphnet_amd.synthetic import FEATURES_ICECUBE86, synthetic_icecube86_raw
from radial_reference import ptr_of, radius_table


@pytest.fixture(scope="module")
def lib():
    from graphnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_class_is_exported_with_the_reference_signature():
    # models/graphs/edges/edges.py:86-90: names, order and defaults; the third argument is radius_graph's max_num_neighbors
    params = list(inspect.signature(g.RadialEdges.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["radius", "columns", "max_num_neighbours"]
    assert [p.default for p in params] == [inspect.Parameter.empty, [0, 1, 2], 32]
    ed = g.RadialEdges(0.5)
    assert (ed._radius, ed._columns, ed._max_num_neighbours) == (0.5, [0, 1, 2], 32)
    ed = g.RadialEdges(2.0, columns=[4, 0], max_num_neighbours=8)
    assert (ed._radius, ed._columns, ed._max_num_neighbours) == (2.0, [4, 0], 8)
    assert isinstance(ed, g.Model)


def _call(lib, cap=32, D=3, r=1.0, ldx=7, cols=(0, 1, 2)):
    # null device pointers throughout: every case must be rejected on the host, before any launch
    c = (ctypes.c_int32 * max(len(cols), 1))(*cols)
    return lib.gn_radius_graph(None, ldx, ctypes.cast(c, ctypes.c_void_p), D, r, None, None, 1, 10, cap, None, None, None,
                               None)


@pytest.mark.parametrize("bad", [dict(cap=0), dict(cap=33), dict(D=0), dict(D=9, cols=(0,) * 9), dict(r=0.0), dict(r=-1.0),
                                 dict(r=float("nan")), dict(r=float("inf")), dict(cols=(0, 7, 2)), dict(cols=(0, 1, 9)),
                                 dict()])                     # the last one: valid shape, plan == NULL
def test_entry_rejects_bad_arguments_without_launching(lib, bad):
    from graphnet_amd import _lib
    assert "gn_radius_graph" in _lib.SIGNATURES and hasattr(lib, "gn_radius_graph")
    rc = _call(lib, **bad)
    assert rc != 0 and b"gn_radius_graph" in lib.gn_last_error()


def test_entry_names_what_it_rejects(lib):
    assert _call(lib, cols=(0, 7, 2)) != 0 and b"column out of range" in lib.gn_last_error()
    assert _call(lib) != 0 and b"plan" in lib.gn_last_error()
    assert _call(lib, r=float("nan")) != 0 and b"radius" in lib.gn_last_error()
    assert lib.gn_radius_work_ints(3, 1000) >= 1 + 1000 // 64 + 3 and lib.gn_radius_work_ints(-1, 0) < 0


def _graph_definition():
    return g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86,
                             edge_definition=g.RadialEdges(0.25, columns=[2, 0, 1], max_num_neighbours=12))


def test_cpu_data_records_the_parameters_through_collate_and_select():
    raw, ptr, _ = synthetic_icecube86_raw(5, seed=3)
    gd = _graph_definition()
    graphs = [gd(raw[ptr[b]:ptr[b + 1]].astype(np.float64), FEATURES_ICECUBE86) for b in range(5)]
    want = (0.25, [2, 0, 1], 12)            # 0.25 is exact in the float32 tensor it travels through once batched
    for d in graphs:
        assert d.edge_index is None and "knn_k" not in d and "mink_k" not in d
        assert all(name in d for name in RADIAL_RECORD)
        assert radial_record(d) == want
    b = g.collate_fn(graphs)
    assert "edge_index" not in b.keys() and b.num_graphs == 5
    assert radial_record(b) == want
    assert tuple(b.radial_r.shape) == (5,) and len(b.radial_columns) == 5      # per-event rows, as knn_k / knn_columns
    s = select_events(b, [1, 3, 4])
    assert "edge_index" not in s.keys() and s.num_graphs == 3
    assert radial_record(s) == want and tuple(s.radial_max.shape) == (3,)
    assert radial_record(s.to("cpu")) == want
    assert radial_record(g.Data(x=torch.zeros(2, 7))) is None


def test_model_config_round_trips_through_yaml(tmp_path):
    gd = _graph_definition()
    path = str(tmp_path / "graph.yml")
    gd.save_config(path)
    text = open(path).read()
    assert "RadialEdges" in text and "radius: 0.25" in text and "max_num_neighbours: 12" in text
    gd2 = g.Model.from_config(path)
    assert gd2.config.as_dict() == gd.config.as_dict() and gd2.config.dump() == text
    ed = gd2._edge_definition
    assert isinstance(ed, g.RadialEdges)
    assert (ed._radius, ed._columns, ed._max_num_neighbours) == (0.25, [2, 0, 1], 12)


@pytest.mark.parametrize("who", ["DynEdgeJINST", "DynEdgeTITO", "ParticleNeT"])
def test_sibling_backbones_name_the_record_they_do_not_build(who):
    # the check runs where the backbone would otherwise build k-NN; reached here through the helper they all call
    from graphnet_amd.gnn import _no_radial_record
    d = g.RadialEdges(0.5)(g.Data(x=torch.zeros(4, 7)))
    with pytest.raises(NotImplementedError, match="RadialEdges"):
        _no_radial_record(d, None, who)
    _no_radial_record(d, torch.zeros(2, 0, dtype=torch.int64), who)           # with an edge_index: nothing to refuse
    _no_radial_record(g.Data(x=torch.zeros(4, 7)), None, who)


def test_numpy_reference_agrees_with_a_kd_tree_on_an_integer_grid():
    """Integer coordinates: every d2 is an exact integer and r2 = 2.25 is none, so fp64 and fp32 agree and
    ``query_ball_point`` (closed ball, fp64) gives the same sets as the strict fp32 rule."""
    from scipy.spatial import cKDTree
    gen = torch.Generator().manual_seed(5)
    sizes = [300, 90]
    n = sum(sizes)
    x = torch.randint(0, 4, (n, 3), generator=gen).float()
    ptr = ptr_of(sizes)
    nbr, deg = radius_table(x, ptr, [0, 1, 2], 1.5, 300)                       # cap >= n: nothing is cut
    assert int(deg.max()) <= 299 and int(deg.max()) > 32
    for b in range(2):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        pts = x[lo:hi].numpy().astype(np.float64)
        for i, found in enumerate(cKDTree(pts).query_ball_point(pts, 1.5)):
            want = {j + lo for j in found if j != i}
            row = nbr[lo + i]
            assert set(row[row >= 0].tolist()) == want and int(deg[lo + i]) == len(want)
