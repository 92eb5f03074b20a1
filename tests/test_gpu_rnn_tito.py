"""GPU: ``RNN_TITO`` = ``Node_RNN`` + ``DynEdgeTITO`` on the bundled prometheus events, configured as the reference's example
(``examples/04_training/05_train_RNN_TITO.py``: no charge column, ``time_series_columns=[4, 3]``), against the float64 GRU
reference (``dom_series_reference.gru_reference``) chained into ``oracle.tito_oracle.DynEdgeTITOOracle``.  As in
test_gpu_tito.py the graph is the device's own (checked bit for bit) and the max-aggregation, pooling and dropout decisions
are teacher-forced.  fp32: latent under 1e-4, every parameter gradient under 2e-3; bf16: latent under 2e-2."""
import os

import numpy as np
import pytest
import torch

import dom_series_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["sensor_pos_x", "sensor_pos_y", "sensor_pos_z", "t"]
KW = dict(dyntrans_layer_sizes=[(32, 32)], post_processing_layer_sizes=[32], readout_layer_sizes=[32, 16], n_head=4,
          features_subset=[0, 1, 2, 3])


def rel_err(a, b) -> float:
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _graph_definition():
    import graphnet_amd as g
    return g.KNNGraph(g.Prometheus(), node_definition=g.NodeAsDOMTimeSeries(
        keys=NAMES, id_columns=NAMES[:3], time_column="t", charge_column="None"), input_feature_names=NAMES)


def _events(count=50):
    ev = np.load(os.path.join(GOLDEN, "reference_events.npz"))
    ptr = ev["prometheus_ptr"]
    return [ev["prometheus_x"][ptr[i]:ptr[i + 1]] for i in range(count)]


@pytest.fixture(scope="module")
def setup(oracle):
    """Model, device batch, and everything of the reference side that does not depend on the compute mode."""
    import graphnet_amd as g
    from oracle import tito_oracle
    gd = _graph_definition()
    assert gd.nb_outputs == 5
    events = _events()
    b = gd.batch_from_raw(events, NAMES, device=DEV)
    h = gd.batch_from_raw(events, NAMES, device="cpu")            # the host path: equal, tests/test_gpu_dom_series.py
    torch.manual_seed(23)
    m = g.RNN_TITO(gd.nb_outputs, [4, 3], **KW).to(DEV)
    ref = tito_oracle.DynEdgeTITOOracle(69, **{k: v for k, v in KW.items() if k != "features_subset"}).eval()
    ref.load_state_dict({k[len("_dynedge_tito."):]: v.cpu() for k, v in m.state_dict().items() if k.startswith("_dynedge_tito.")})
    rows, series_ptr, dom_ptr = h.x.numpy(), h.series_ptr.numpy(), h.dom_ptr.numpy()
    dom = torch.from_numpy(R.dom_rows_reference(rows, series_ptr, 4)).float()
    batch = torch.from_numpy(np.repeat(np.arange(len(dom_ptr) - 1), np.diff(dom_ptr)))
    ei = oracle.knn_graph(dom, 8, batch, [0, 1, 2, 3])
    return dict(m=m, ref=ref, b=b, rows=rows, series_ptr=series_ptr, dom=dom, batch=batch, ei=ei, n_pulses=h.n_pulses)


def _reference_pass(s, tr, drop, w):
    """float64 GRU -> fp32 oracle with the device's decisions replayed; returns (latent, GRU module, GRU output)."""
    s["ref"].zero_grad()
    params = {k: v.detach().cpu() for k, v in s["m"]._rnn._rnn.named_parameters()}
    rnn_out, gru = R.gru_reference(s["rows"][:, [4, 3]], s["series_ptr"], params, num_layers=2)
    x = torch.cat([s["dom"], rnn_out.float()], dim=1)
    yo, tro = s["ref"](x, s["ei"], s["batch"], s["n_pulses"], return_trace=True, drop=drop,
                       forced_max_rank=[r.cpu() for r in tr["max_arg_rank"]],
                       forced_pool_arg={k: v.cpu() for k, v in tr["pool_arg"].items()})
    if w is not None:
        (yo * w).sum().backward()
    return yo, tro, gru, rnn_out


def test_rnn_tito_fp32_forward_backward(setup):
    from graphnet_amd import ops
    s = setup
    m = s["m"].set_backend(dtype="fp32")
    m.train()
    m.zero_grad()
    seen = []
    hook = m._rnn.register_forward_hook(lambda mod, args, out: seen.append(out.x.detach().clone()))
    y, tr = m(s["b"], return_trace=True)
    hook.remove()
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(2))
    (y * w.to(DEV)).sum().backward()
    assert len(tr["dropout_seeds"]) == 1                           # DynEdgeTITO's default dropout 0.1 is live in training
    yo, tro, gru, rnn_out = _reference_pass(s, tr, (ops.drop_thresh(0.1), tr["dropout_seeds"]), w)
    assert torch.equal(tr["graph"].edge_index().cpu(), s["ei"])    # k-NN on features_subset of the DOM rows, bit-exact
    assert max(tro["max_gap"]) < 1e-5 and tro["pool_gap"] < 1e-5, (tro["max_gap"], tro["pool_gap"])
    assert rel_err(seen[0][:, :5], s["dom"]) < 1e-6 and rel_err(seen[0][:, 5:], rnn_out.detach()) < 1e-4
    print(f"latent {rel_err(y, yo.detach()):.2e}")
    assert rel_err(y, yo.detach()) < 1e-4
    for name, p in m.named_parameters():
        if name.startswith("_rnn._rnn."):
            short = name[len("_rnn._rnn."):]
            if short.endswith("_l1"):
                assert p.grad is None, name
                continue
            want = gru.get_parameter(short).grad
        else:
            want = s["ref"].get_parameter(name[len("_dynedge_tito."):]).grad
        assert p.grad is not None, name
        print(f"grad {name} {rel_err(p.grad, want):.2e}")
        assert rel_err(p.grad, want) < 2e-3, name


def test_rnn_tito_bf16_same_gru_bits_and_latent(setup):
    s = setup
    m = s["m"].eval()
    seen = []
    hook = m._rnn.register_forward_hook(lambda mod, args, out: seen.append(out.x.detach().clone()))
    with torch.no_grad():
        m.set_backend(dtype="fp32")(s["b"])
        y, tr = m.set_backend(dtype="bf16")(s["b"], return_trace=True)
    hook.remove()
    assert torch.equal(seen[1], seen[0]) and seen[0].shape == (1511, 69)    # the GRU is fp32 in both modes: bit for bit
    yo, tro, _, _ = _reference_pass(s, tr, None, None)
    assert max(tro["max_gap"]) < 2e-2 and tro["pool_gap"] < 2e-2, (tro["max_gap"], tro["pool_gap"])
    print(f"bf16 latent {rel_err(y, yo.detach()):.2e}")
    assert rel_err(y, yo.detach()) < 2e-2


def test_rnn_tito_state_dict_round_trip_and_eval_mode(setup):
    import graphnet_amd as g
    s = setup
    m = s["m"].set_backend(dtype="fp32").eval()
    with torch.no_grad():
        y = m(s["b"])
        assert y.shape == (50, 16) and torch.equal(y, m(s["b"]))    # eval: deterministic, no dropout
        torch.manual_seed(99)
        m2 = g.RNN_TITO(5, [4, 3], **KW)
        m2.load_state_dict(m.state_dict())
        assert torch.equal(m2.to(DEV).set_backend(dtype="fp32").eval()(s["b"]), y)
    torch.manual_seed(5)
    y1 = m.train()(s["b"])
    assert not torch.equal(y1.detach(), y)                          # train: dropout inside DynEdgeTITO
