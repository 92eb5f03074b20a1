"""CPU: the host side of ``MinkowskiKNNEdges`` - the public class, the C entry's argument validation, the record a CPU
``Data`` carries to the backbone, and the config round trip (no device ops)."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import graphnet_amd as g
from graphnet_amd.data import select_events
from graphnet_amd.graphs import MINKOWSKI_RECORD, minkowski_record
from graphnet_amd.synthetic import FEATURES_ICECUBE86, synthetic_icecube86_raw


@pytest.fixture(scope="module")
def lib():
    from graphnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_class_is_exported_with_the_reference_signature():
    # models/graphs/edges/minkowski.py:40-47: names, order and defaults
    params = list(inspect.signature(g.MinkowskiKNNEdges.__init__).parameters.values())[1:]
    assert [p.name for p in params] == ["nb_nearest_neighbours", "c", "time_like_weight", "space_coords", "time_coord"]
    empty = inspect.Parameter.empty
    assert [p.default for p in params] == [empty, empty, 1.0, None, 3]
    ed = g.MinkowskiKNNEdges(8, 0.3)
    assert (ed.nb_nearest_neighbours, ed.c, ed.time_like_weight, ed.space_coords, ed.time_coord) == (8, 0.3, 1.0, [0, 1, 2], 3)
    ed = g.MinkowskiKNNEdges(4, c=1.0, time_like_weight=2.0, space_coords=[4, 0], time_coord=5)
    assert (ed.space_coords, ed.time_coord, ed.time_like_weight) == ([4, 0], 5, 2.0)
    assert isinstance(ed, g.Model)


def _call(lib, k=8, DS=3, time_col=3, ldx=7, cols=None):
    # null device pointers throughout: every case must be rejected on the host, before any launch
    return lib.gn_minkowski_knn_graph(None, ldx, cols, DS, time_col, 1.0, 1.0, None, None, 1, 10, k, None, None)


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=33), dict(DS=0), dict(DS=8), dict(time_col=7), dict(time_col=9)])
def test_entry_rejects_bad_arguments_without_launching(lib, bad):
    from graphnet_amd import _lib
    assert "gn_minkowski_knn_graph" in _lib.SIGNATURES and hasattr(lib, "gn_minkowski_knn_graph")
    rc = _call(lib, **bad)
    assert rc != 0 and b"gn_minkowski_knn_graph" in lib.gn_last_error()


def test_entry_rejects_a_space_column_out_of_range_and_a_missing_plan(lib):
    cols = (ctypes.c_int32 * 3)(0, 7, 2)
    rc = _call(lib, cols=ctypes.cast(cols, ctypes.c_void_p))
    assert rc != 0 and b"gn_minkowski_knn_graph" in lib.gn_last_error() and b"space column" in lib.gn_last_error()
    cols = (ctypes.c_int32 * 3)(0, 1, 2)
    rc = _call(lib, cols=ctypes.cast(cols, ctypes.c_void_p))                   # valid shape, tile_ptr == NULL
    assert rc != 0 and b"gn_minkowski_knn_graph" in lib.gn_last_error() and b"plan" in lib.gn_last_error()


def _graph_definition():
    return g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86,
                             edge_definition=g.MinkowskiKNNEdges(6, c=0.3, time_like_weight=2.5, space_coords=[2, 0, 1],
                                                                 time_coord=3))


def test_cpu_data_records_the_parameters_through_collate_and_select():
    raw, ptr, _ = synthetic_icecube86_raw(5, seed=3)
    gd = _graph_definition()
    graphs = [gd(raw[ptr[b]:ptr[b + 1]].astype(np.float64), FEATURES_ICECUBE86) for b in range(5)]
    want = (6, float(np.float32(0.3)), 2.5, 3, [2, 0, 1])

    def rounded(rec):               # c travels through a float32 tensor once the events are batched
        return (rec[0], float(np.float32(rec[1])), float(np.float32(rec[2])), rec[3], rec[4])

    for d in graphs:
        assert d.edge_index is None and "knn_k" not in d
        assert all(name in d for name in MINKOWSKI_RECORD)
        assert rounded(minkowski_record(d)) == want
    b = g.collate_fn(graphs)
    assert "edge_index" not in b.keys() and b.num_graphs == 5
    assert rounded(minkowski_record(b)) == want
    assert tuple(b.mink_k.shape) == (5,) and len(b.mink_space_coords) == 5      # per-event rows, as knn_k / knn_columns
    s = select_events(b, [1, 3, 4])
    assert "edge_index" not in s.keys() and s.num_graphs == 3
    assert rounded(minkowski_record(s)) == want and tuple(s.mink_k.shape) == (3,)
    assert rounded(minkowski_record(s.to("cpu"))) == want
    assert minkowski_record(g.Data(x=torch.zeros(2, 7))) is None


def test_model_config_round_trips_through_yaml(tmp_path):
    gd = _graph_definition()
    path = str(tmp_path / "graph.yml")
    gd.save_config(path)
    text = open(path).read()
    assert "MinkowskiKNNEdges" in text and "time_like_weight: 2.5" in text
    gd2 = g.Model.from_config(path)
    assert gd2.config.as_dict() == gd.config.as_dict() and gd2.config.dump() == text
    ed = gd2._edge_definition
    assert isinstance(ed, g.MinkowskiKNNEdges)
    assert (ed.nb_nearest_neighbours, ed.c, ed.time_like_weight, ed.space_coords, ed.time_coord) == (6, 0.3, 2.5, [2, 0, 1], 3)
