"""CPU: the ``NodeAsDOMTimeSeries`` contract and the surface of ``Node_RNN`` / ``RNN_TITO``.  The loop-per-DOM restatement
(``dom_series_reference.py``) equals what the reference's ``_construct_nodes`` recorded
(``golden/dom_time_series_expected.npz``), the product's vectorised host path equals the restatement, the classes have the
reference's constructors and state-dict keys, and the new C entries refuse bad arguments without a launch.  The device
paths are compared against the same restatement in tests/test_gpu_dom_series.py and tests/test_gpu_gru.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import dom_series_reference as R
import graphnet_amd as g
from graphnet_amd import _lib
from graphnet_amd.graphs import dom_time_series_host
from graphnet_amd.synthetic import FEATURES_ICECUBE86

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("prometheus", 50, 1511, 12), ("deepcore", 5, 38, 7), ("upgrade", 2, 154, 21), ("deepcore_none", 5, 38, 7)]


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "dom_time_series_expected.npz"))


def _case(recorded, name):
    return (recorded[name + "_x"], recorded[name + "_ptr"], recorded[name + "_rows"], int(recorded[name + "_charge_col"]))


def _ties_sorted(rows):
    """Rows of one event with every run of equal (id tuple, time) put in one canonical order; number of rows in such runs."""
    rows, n, affected, i = rows.copy(), len(rows), 0, 0
    while i < n:
        j = i + 1
        while j < n and R.same(rows[j, :4], rows[i, :4]):
            j += 1
        if j - i > 1:
            affected += j - i
            block = rows[i:j]
            rows[i:j] = block[np.lexsort(block.T[::-1])]
        i = j
    return rows, affected


# ------------------------------------------------------------------------------ 1. restatement == the reference's results
@pytest.mark.parametrize("name,events,series,longest", CASES)
def test_restatement_equals_the_recorded_reference_results(recorded, name, events, series, longest):
    """Measured on the fixtures: no row lies in a run of equal (DOM, time), so the tie rule decides nothing there; the
    charge column (the reference's fp32 ``np.power`` against the contract's fp64 power rounded to fp32) differs by at most
    1 ulp (deepcore 1, upgrade 1; without a charge column the ones are exact).  Asserted: that measured 1 plus one ulp for
    another libm."""
    x, ptr, exp, charge_col = _case(recorded, name)
    assert len(ptr) - 1 == events and exp.dtype == np.float32 and exp.shape == (len(x), x.shape[1] + (charge_col < 0) + 1)
    got, series_ptr, dom_ptr, got_longest = R.series_batch(x, ptr, [0, 1, 2], 3, charge_col)
    assert (len(series_ptr) - 1, got_longest, int(dom_ptr[-1])) == (series, longest, series)
    assert np.array_equal(np.flatnonzero(exp[:, -1]), series_ptr[:-1])
    affected = 0
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        a, na = _ties_sorted(got[lo:hi])
        b, nb = _ties_sorted(exp[lo:hi])
        assert na == nb
        affected += na
        keep = [c for c in range(a.shape[1]) if c != charge_col]
        assert R.same(a[:, keep], b[:, keep])
        if charge_col >= 0:
            ulps = R.ulp_distance(a[:, charge_col], b[:, charge_col])
            print(f"{name}: charge column within {ulps} ulp")
            assert ulps <= 2
    assert affected == 0


# ------------------------------------------------------------------------------ 2. product host path == restatement
def _host_batch(x, ptr, id_cols, time_col, charge_col):
    return np.concatenate([dom_time_series_host(x[lo:hi], id_cols, time_col, charge_col) for lo, hi in zip(ptr[:-1], ptr[1:])])


def test_host_path_equals_restatement_on_the_recorded_events(recorded):
    for name, *_ in CASES:
        x, ptr, _, charge_col = _case(recorded, name)
        assert R.same(_host_batch(x, ptr, [0, 1, 2], 3, charge_col), R.series_batch(x, ptr, [0, 1, 2], 3, charge_col)[0])


def test_host_path_equals_restatement_on_the_generated_batch():
    x, ptr = R.shapes_batch()
    exp, series_ptr, dom_ptr, longest = R.series_batch(x, ptr, [0, 1, 2], 3, 4)
    assert np.diff(dom_ptr).tolist() == [2, 2, 10, 1, 40, 80, 83, 82, 539, 552] and longest == 40
    assert R.same(_host_batch(x, ptr, [0, 1, 2], 3, 4), exp)
    assert R.same(_host_batch(x, ptr, [2, 0], 3, -1), R.series_batch(x, ptr, [2, 0], 3, -1)[0])


def test_host_path_ties_zeros_and_nans():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[1, 0.0, 5, 0.5, 0], [1, -0.0, 5, 0.5, 1], [nan, 0, 7, 2.0, 2], [nan, 0, 7, -0.0, 3], [1, 0, 5, 0.0, 4],
                  [1, 0, -inf, 3, 5], [nan, 0, 7, 0.0, 6], [1, 0, 5, 0.5, 7]], dtype=np.float32)
    exp, lens = R.event_rows(x, [0, 1, 2], 3, -1)
    assert lens == [1, 4, 3]
    assert exp[:, 4].tolist() == [5, 4, 0, 1, 7, 3, 6, 2]        # equal times inside a DOM: by pulse index; -0.0 == +0.0
    assert R.same(dom_time_series_host(x, [0, 1, 2], 3, -1), exp)
    x[3, 3] = nan                                                # one NaN time: last in its DOM, the whole column NaN
    exp, _ = R.event_rows(x, [0, 1, 2], 3, 4)
    assert np.isnan(exp[:, 3]).all() and exp[:, 5].tolist() == [1, 1, 0, 0, 0, 1, 0, 0]
    got = dom_time_series_host(x, [0, 1, 2], 3, 4)
    assert R.same(got, exp) and got[-1, 4] == 1000.0             # 10^3; the NaN-time pulse is the DOM's last row
    assert dom_time_series_host(np.zeros((0, 5), np.float32), [0, 1, 2], 3, 4).shape == (0, 6)


# ------------------------------------------------------------------------------ 3. class surface
def test_node_definition_has_the_reference_arguments_and_names():
    sig = inspect.signature(g.NodeAsDOMTimeSeries.__init__)
    assert list(sig.parameters)[1:] == ["keys", "id_columns", "time_column", "charge_column", "max_activations"]
    assert sig.parameters["keys"].default == ["dom_x", "dom_y", "dom_z", "dom_time", "charge"]
    assert sig.parameters["id_columns"].default == ["dom_x", "dom_y", "dom_z"]
    assert (sig.parameters["time_column"].default, sig.parameters["charge_column"].default) == ("dom_time", "charge")
    assert sig.parameters["max_activations"].default is None
    nd = g.NodeAsDOMTimeSeries(max_activations=7)
    assert nd._max_activations == 7 and nd.nb_outputs == 6
    assert nd._output_feature_names == ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "new_node_col"]
    # the example: no charge column; the NAMES stay input + new_node_col although the matrix is one wider
    keys = ["dom_x", "dom_y", "dom_z", "dom_time"]
    nd = g.NodeAsDOMTimeSeries(keys=keys, id_columns=keys[:3], time_column="dom_time", charge_column="None")
    assert nd._charge_index is None and nd.nb_outputs == 5 and nd._output_feature_names == keys + ["new_node_col"]


def test_cpu_tensor_takes_the_host_path(recorded):
    x, ptr, _, charge_col = _case(recorded, "deepcore")
    keys = ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "rde", "pmt_area"]
    nd = g.NodeAsDOMTimeSeries(keys=keys)
    graph, names = nd(torch.from_numpy(x[ptr[0]:ptr[1]]))
    assert names == keys + ["new_node_col"] and graph.x.dtype == torch.float32
    assert R.same(graph.x.numpy(), R.event_rows(x[ptr[0]:ptr[1]], [0, 1, 2], 3, 4)[0])
    rows, series_ptr, dom_ptr = nd.series_batch(torch.from_numpy(x), torch.from_numpy(ptr))
    exp, exp_sp, exp_dp, _ = R.series_batch(x, ptr, [0, 1, 2], 3, 4)
    assert R.same(rows.numpy(), exp) and np.array_equal(series_ptr.numpy(), exp_sp) and np.array_equal(dom_ptr.numpy(), exp_dp)


def test_batch_from_raw_on_the_host_carries_the_series():
    ev = np.load(os.path.join(GOLDEN, "reference_events.npz"))
    ptr = ev["deepcore_ptr"]
    events = [ev["deepcore_x"][ptr[i]:ptr[i + 1]] for i in range(5)]
    gd = g.KNNGraph(g.IceCube86(), node_definition=g.NodeAsDOMTimeSeries(keys=FEATURES_ICECUBE86),
                    input_feature_names=FEATURES_ICECUBE86)
    assert gd.nb_outputs == len(FEATURES_ICECUBE86) + 1
    b = gd.batch_from_raw(events, FEATURES_ICECUBE86, device="cpu")
    per_event = [gd(e.copy(), FEATURES_ICECUBE86) for e in events]
    assert torch.equal(b.x, torch.cat([d.x for d in per_event]))
    n = sum(len(e) for e in events)
    assert tuple(b.x.shape) == (n, len(FEATURES_ICECUBE86) + 1) and b.n_pulses.tolist() == [len(e) for e in events]
    assert b.ptr.tolist() == ptr[:6].tolist() and b.batch.tolist() == np.repeat(np.arange(5), np.diff(ptr[:6])).tolist()
    assert int(b.series_ptr[-1]) == n and int(b.dom_ptr[-1]) == len(b.series_ptr) - 1 == 38
    assert np.array_equal(np.flatnonzero(b.x[:, -1].numpy()), b.series_ptr[:-1].numpy())


# ------------------------------------------------------------------------------ 4. constructors and state dicts
def test_node_rnn_and_rnn_tito_have_the_reference_constructors():
    p = inspect.signature(g.Node_RNN.__init__).parameters
    assert list(p)[1:] == ["nb_inputs", "hidden_size", "num_layers", "time_series_columns", "nb_neighbours", "features_subset",
                           "dropout", "embedding_dim"]
    assert (p["nb_neighbours"].default, p["features_subset"].default, p["dropout"].default, p["embedding_dim"].default) == \
        (8, None, 0.5, 0)
    p = inspect.signature(g.RNN_TITO.__init__).parameters
    assert list(p)[1:] == ["nb_inputs", "time_series_columns", "nb_neighbours", "rnn_layers", "rnn_hidden_size", "rnn_dropout",
                           "features_subset", "dyntrans_layer_sizes", "post_processing_layer_sizes", "readout_layer_sizes",
                           "global_pooling_schemes", "embedding_dim", "n_head", "use_global_features",
                           "use_post_processing_layers"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[3:])
    assert (p["rnn_layers"].default, p["rnn_hidden_size"].default, p["rnn_dropout"].default, p["embedding_dim"].default,
            p["n_head"].default, p["global_pooling_schemes"].default) == (2, 64, 0.5, None, 16, ["max"])
    rnn = g.Node_RNN(2, 64, 2, [4, 3])
    assert rnn.nb_outputs == 69 and rnn.nb_inputs == 2
    assert g.Node_RNN(2, 64, 1, [4, 3], embedding_dim=16)._rnn.weight_ih_l0.shape == (192, 32)


def test_rnn_tito_state_dict_is_the_reference_composition():
    m = g.RNN_TITO(5, [4, 3], dyntrans_layer_sizes=[(32, 32)], n_head=4)           # embedding_dim=None: no embedding
    tito = g.DynEdgeTITO(nb_inputs=69, dyntrans_layer_sizes=[(32, 32)], n_head=4)
    gru = torch.nn.GRU(2, 64, 2)
    want = ["_rnn._rnn." + k for k in gru.state_dict()] + ["_dynedge_tito." + k for k in tito.state_dict()]
    assert sorted(m.state_dict()) == sorted(want)
    assert sorted(k for k in want if k.startswith("_rnn.")) == sorted(
        f"_rnn._rnn.{w}_{s}_l{k}" for w in ("weight", "bias") for s in ("ih", "hh") for k in (0, 1))
    sd = dict(m.state_dict())
    sd.update({"_rnn._rnn." + k: v for k, v in gru.state_dict().items()})
    m.load_state_dict(sd)
    assert torch.equal(m._rnn._rnn.weight_hh_l1, gru.weight_hh_l1) and m.nb_outputs == 128 and m.nb_inputs == 5
    assert m._dynedge_tito._graph_columns == [0, 1, 2, 3]
    assert g.RNN_TITO(5, [4, 3], features_subset=[0, 1, 2], dyntrans_layer_sizes=[(32, 32)], n_head=4) \
        ._dynedge_tito._graph_columns == [0, 1, 2]
    with pytest.raises(RuntimeError, match="HIP"):
        m(g.Batch(x=torch.zeros(4, 6), n_pulses=torch.tensor([4])))                 # CPU tensors: no fallback


# ------------------------------------------------------------------------------ 5. C entries: bad arguments, no launch
def test_new_entries_reject_bad_arguments_without_a_launch():
    L = _lib.lib()
    assert L.gn_gru_supported(2, 64) == 1 and L.gn_gru_supported(32, 64) == 1 and L.gn_gru_supported(2, 4) == 1
    assert [L.gn_gru_supported(*a) for a in ((0, 64), (33, 64), (2, 0), (2, 66), (2, 68), (2, 128))] == [0] * 6
    assert L.gn_gru_saved_floats(10, 64) == 3200 and L.gn_gru_bwd_work_floats(10, 2, 65) == -1
    assert L.gn_gru_bwd_work_floats(10, 2, 64) >= 2 * 10 * 192 + 10 * 4
    assert L.gn_dom_time_series_work_ints(3, 100) == 100 + 3 + 2 and L.gn_dom_time_series_work_ints(-1, 1) == -1
    big = L.gn_percentile_lds_max() + 1
    assert L.gn_dom_time_series_work_ints(1, big) == 6 * big + 1 + 2
    buf = (ctypes.c_float * 64)()
    ints = (ctypes.c_int32 * 64)(0, 2)
    ids = (ctypes.c_int32 * 9)(0, 1, 2, 0)
    p, q, i = ctypes.addressof(buf), ctypes.addressof(ints), ctypes.addressof(ids)

    def dts(**kw):
        a = dict(x=p, ldx=4, F=4, N=2, ptr=q, B=1, ids=i, C=3, t=3, ch=-1, out=p, ldo=6, sp=q, dp=q, work=q)
        a.update(kw)
        return L.gn_dom_time_series(a["x"], a["ldx"], a["F"], a["N"], a["ptr"], a["B"], a["ids"], a["C"], a["t"], a["ch"],
                                    a["out"], a["ldo"], a["sp"], a["dp"], a["work"], None)
    for bad in (dict(C=0), dict(C=9), dict(t=4), dict(t=2), dict(C=4), dict(ldo=5), dict(ch=3), dict(ch=4), dict(F=5),
                dict(N=-1), dict(B=-1), dict(sp=None), dict(ptr=None), dict(x=None), dict(work=None), dict(ids=None)):
        assert dts(**bad) != 0, bad
        assert b"gn_dom_time_series" in L.gn_last_error()

    def fwd(**kw):
        a = dict(xs=p, ldx=2, T=2, I=2, sp=q, M=1, H=64, wih=p, whh=p, bih=p, bhh=p, out=p, saved=None)
        a.update(kw)
        return L.gn_gru_series_fwd(a["xs"], a["ldx"], a["T"], a["I"], a["sp"], a["M"], a["H"], a["wih"], a["whh"], a["bih"],
                                   a["bhh"], a["out"], a["saved"], None)
    for bad in (dict(H=65), dict(H=128), dict(I=33), dict(I=0), dict(ldx=1), dict(M=3), dict(T=-1), dict(wih=None),
                dict(bhh=None), dict(xs=None), dict(out=None), dict(saved=p + 4)):
        assert fwd(**bad) != 0, bad
        assert b"gn_gru_series_fwd" in L.gn_last_error()

    def bwd(**kw):
        a = dict(dout=p, saved=p, xs=p, ldx=2, T=2, I=2, sp=q, M=1, H=64, whh=p, dwih=p, dbih=p, dwhh=p, dbhh=p, work=p)
        a.update(kw)
        return L.gn_gru_series_bwd(a["dout"], a["saved"], a["xs"], a["ldx"], a["T"], a["I"], a["sp"], a["M"], a["H"], a["whh"],
                                   a["dwih"], a["dbih"], a["dwhh"], a["dbhh"], a["work"], None)
    for bad in (dict(H=63), dict(I=40), dict(M=3), dict(ldx=1), dict(whh=None), dict(dwih=None), dict(saved=None),
                dict(work=None), dict(dout=None), dict(work=p + 4)):
        assert bwd(**bad) != 0, bad
        assert b"gn_gru_series_bwd" in L.gn_last_error()
    for bad in ((p, 4, 4, 2, q, 3, 3, p, 4), (p, 4, 4, 2, q, 1, 4, p, 4), (p, 4, 4, 2, q, 1, -1, p, 4), (p, 4, 4, 2, q, 1, 3, p, 3),
                (p, 4, 5, 2, q, 1, 3, p, 5), (None, 4, 4, 2, q, 1, 3, p, 4), (p, 4, 4, 2, None, 1, 3, p, 4)):
        assert L.gn_dom_series_summary(*bad, None) != 0, bad
        assert b"gn_dom_series_summary" in L.gn_last_error()
