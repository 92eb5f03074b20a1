"""GPU: ``gn_dom_time_series`` against the loop-per-DOM restatement (``dom_series_reference.py``).  Exact, NaN equal to NaN;
the one exception is the charge column, where the fp32 bit pattern may differ by one because the device ``pow`` is not
numpy's."""
import os

import numpy as np
import pytest
import torch

import dom_series_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _device(x, ptr, id_cols, time_col, charge_col, **kw):
    from graphnet_amd import ops
    rows, series_ptr, dom_ptr = ops.dom_time_series(x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV),
                                                    torch.as_tensor(np.asarray(ptr), dtype=torch.int32).to(DEV), id_cols,
                                                    time_col, charge_col, **kw)
    return rows, series_ptr.cpu().numpy(), dom_ptr.cpu().numpy()


@pytest.fixture(scope="module")
def shapes():
    from graphnet_amd import _lib
    lds_max = int(_lib.lib().gn_percentile_lds_max())
    x, ptr = R.shapes_batch(lds_max)
    return lds_max, x, ptr, R.series_batch(x, ptr, [0, 1, 2], 3, 4)


def test_shapes_batch_rows_and_series(shapes):
    """Events of 2, 3, 64 pulses, one DOM, one DOM per pulse, 511 / 512 / 513 and the LDS limit and one more pulse."""
    lds_max, x, ptr, (exp, exp_sp, exp_dp, longest) = shapes
    # what the restatement alone says about this input
    assert np.diff(ptr).tolist() == [2, 3, 64, 40, 40, 511, 512, 513, lds_max, lds_max + 1]
    if lds_max == 4096:
        assert np.diff(exp_dp).tolist() == [2, 2, 10, 1, 40, 80, 83, 82, 539, 552]
    assert np.diff(exp_dp)[3:5].tolist() == [1, 40] and longest == 40 and int(np.diff(exp_sp).min()) == 1
    ties = sum(int((np.diff(exp[a:b, 3]) == 0).sum()) for a, b in zip(exp_sp[:-1], exp_sp[1:]))
    assert ties > 500                                              # equal times inside a DOM: the order is by pulse index
    rows, series_ptr, dom_ptr = _device(x, ptr, [0, 1, 2], 3, 4)
    assert np.array_equal(dom_ptr, exp_dp) and np.array_equal(series_ptr, exp_sp)
    assert R.same_but_charge(rows.cpu().numpy(), exp, 4)
    assert R.same(rows.cpu().numpy()[:, 5], exp[:, 5])             # the tag column: which pulse went where


def test_strided_input_output_pitch_and_no_charge_column(shapes):
    _, x, ptr, _ = shapes
    wide = torch.full((len(x), 11), float("nan"), device=DEV)
    wide[:, 2:8] = torch.from_numpy(x).to(DEV)
    exp, exp_sp, exp_dp, _ = R.series_batch(x, ptr, [2, 0], 3, -1)
    rows, series_ptr, dom_ptr = _device(wide[:, 2:8], ptr, [2, 0], 3, -1, out_pitch=12)
    assert rows.shape == (len(x), 8) and rows.stride(0) == 12
    assert R.same(rows.cpu().numpy(), exp) and np.array_equal(series_ptr, exp_sp) and np.array_equal(dom_ptr, exp_dp)
    assert bool((rows[:, 6] == 1.0).all())


def test_zeros_nans_and_equal_times():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[1, 0.0, 5, 0.5, 0], [1, -0.0, 5, 0.5, 1], [nan, 0, 7, 2.0, 2], [nan, 0, 7, -0.0, 3], [1, 0, 5, 0.0, 4],
                  [1, 0, -inf, 3, 5], [nan, 0, 7, 0.0, 6], [1, 0, 5, 0.5, 7]], dtype=np.float32)
    y = x.copy()
    y[3, 3] = nan                                                  # second event: one NaN time -> the whole column NaN
    both, ptr = np.concatenate([x, y]), [0, 8, 16]
    exp, exp_sp, exp_dp, _ = R.series_batch(both, ptr, [0, 1, 2], 3, -1)
    assert exp[:8, 4].tolist() == [5, 4, 0, 1, 7, 3, 6, 2] and exp[8:, 4].tolist() == [5, 4, 0, 1, 7, 6, 2, 3]
    assert np.isnan(exp[8:, 3]).all() and not np.isnan(exp[:8, 3]).any() and exp_dp.tolist() == [0, 3, 6]
    rows, series_ptr, dom_ptr = _device(both, ptr, [0, 1, 2], 3, -1)
    assert R.same(rows.cpu().numpy(), exp) and np.array_equal(series_ptr, exp_sp) and np.array_equal(dom_ptr, exp_dp)
    exp, _, _, _ = R.series_batch(both, ptr, [0, 1, 2], 3, 4)     # the tag column as charge: 10^0 .. 10^7 exactly
    rows, _, _ = _device(both, ptr, [0, 1, 2], 3, 4)
    assert R.same_but_charge(rows.cpu().numpy(), exp, 4)


def test_empty_batch_and_an_empty_event_in_the_middle(shapes):
    _, x, ptr, _ = shapes
    rows, series_ptr, dom_ptr = _device(torch.zeros((0, 6), device=DEV), [0], [0, 1, 2], 3, 4)
    assert rows.shape == (0, 7) and series_ptr.tolist() == [0] and dom_ptr.tolist() == [0]
    rows, series_ptr, dom_ptr = _device(torch.zeros((0, 6), device=DEV), [0, 0, 0], [0, 1, 2], 3, 4)
    assert rows.shape == (0, 7) and series_ptr.tolist() == [0] and dom_ptr.tolist() == [0, 0, 0]
    cut = [0, 2, 5, 5, 69, 109, 109]                               # events 3 and 6 are empty
    exp, exp_sp, exp_dp, _ = R.series_batch(x[:109], cut, [0, 1, 2], 3, 4)
    assert np.diff(exp_dp).tolist() == [2, 2, 0, 10, 1, 0]
    rows, series_ptr, dom_ptr = _device(x[:109].copy(), cut, [0, 1, 2], 3, 4)
    assert R.same_but_charge(rows.cpu().numpy(), exp, 4) and np.array_equal(series_ptr, exp_sp) and np.array_equal(dom_ptr, exp_dp)


def test_host_path_equals_device_path_on_synthetic_events():
    import graphnet_amd as g
    from graphnet_amd.synthetic import FEATURES_ICECUBE86, synthetic_icecube86_batch
    b = synthetic_icecube86_batch(12, seed=4)
    nd = g.NodeAsDOMTimeSeries(keys=FEATURES_ICECUBE86)
    ptr = b.ptr.to(torch.int32)
    host = nd.series_batch(b.x, ptr)
    dev = nd.series_batch(b.x.to(DEV), ptr.to(DEV))
    assert R.same_but_charge(dev[0].cpu().numpy(), host[0].numpy(), 4)
    assert torch.equal(dev[1].cpu(), host[1]) and torch.equal(dev[2].cpu(), host[2])
    assert int(host[2][-1]) < len(b.x)                             # some DOM saw more than one pulse
    one = nd(b.x[:int(ptr[1])].to(DEV))[0].x                       # the stand-alone call: one event
    assert R.same_but_charge(one.cpu().numpy(), host[0][:int(ptr[1])].numpy(), 4)


def test_batch_from_raw_with_this_node_definition():
    import graphnet_amd as g
    ev = np.load(os.path.join(GOLDEN, "reference_events.npz"))
    ptr = ev["prometheus_ptr"]
    events = [ev["prometheus_x"][ptr[i]:ptr[i + 1]] for i in range(50)]
    names = ["sensor_pos_x", "sensor_pos_y", "sensor_pos_z", "t"]
    gd = g.KNNGraph(g.Prometheus(), node_definition=g.NodeAsDOMTimeSeries(
        keys=names, id_columns=names[:3], time_column="t", charge_column="None"), input_feature_names=names)
    assert gd.nb_outputs == 5
    b = gd.batch_from_raw(events, names, device=DEV)
    h = gd.batch_from_raw(events, names, device="cpu")
    assert b.x.is_cuda and tuple(b.x.shape) == (int(ptr[50]), 6)
    assert torch.equal(b.x.cpu(), h.x) and torch.equal(b.series_ptr.cpu(), h.series_ptr) and torch.equal(b.dom_ptr.cpu(), h.dom_ptr)
    assert b.ptr.tolist() == ptr.tolist() and b.n_pulses.tolist() == np.diff(ptr).tolist()
    assert torch.equal(b.batch.cpu(), h.batch) and int(b.dom_ptr[-1]) == 1511 and b.series_ptr.shape[0] == 1512
    per_event = torch.cat([gd(e.copy(), names).x for e in events[:5]])
    assert torch.equal(b.x[:len(per_event)].cpu(), per_event)
