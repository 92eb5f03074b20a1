"""GPU: the ragged GRU recurrence (``gn_gru_series_fwd`` / ``gn_gru_series_bwd``), ``Node_RNN`` and ``gn_dom_series_summary``
against float64: ``torch.nn.GRU`` on the CPU over ``pack_sequence(enforce_sorted=False)``, output ``[-1][0]``, which is
literally the reference's call (``dom_series_reference.gru_reference``).  fp32 against float64: forward under 1e-4, the four
gradients under 2e-3, both relative to the largest reference entry - the fp32 gates of test_gpu_tito.py."""
import numpy as np
import pytest
import torch

import dom_series_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
LENGTHS = [1, 2, 63, 64, 65, 300, 1, 1, 7]
NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def rel_err(a, b) -> float:
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _problem(I, H, lengths, seed=0):
    gen = torch.Generator().manual_seed(seed + 1000 * I + H)
    T = sum(lengths)
    xs = torch.randn(T, I, generator=gen)
    params = {"weight_ih_l0": torch.randn(3 * H, I, generator=gen) * 0.5, "weight_hh_l0": torch.randn(3 * H, H, generator=gen) / H ** 0.5,
              "bias_ih_l0": torch.randn(3 * H, generator=gen) * 0.3, "bias_hh_l0": torch.randn(3 * H, generator=gen) * 0.3}
    series_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    dout = torch.randn(len(lengths), H, generator=gen)
    return xs, params, series_ptr, dout


def _device_pass(xs, params, series_ptr, dout):
    from graphnet_amd import ops
    p = [params[k].to(DEV) for k in NAMES]
    sp = torch.from_numpy(series_ptr).to(DEV)
    out, saved = ops.gru_series_fwd(xs.to(DEV), sp, *p)
    grads = ops.gru_series_bwd(dout.to(DEV), saved, xs.to(DEV), sp, p[1])
    return out, dict(zip(("weight_ih_l0", "bias_ih_l0", "weight_hh_l0", "bias_hh_l0"), grads))


@pytest.mark.parametrize("I,H", [(2, 64), (32, 64), (2, 4), (3, 20), (32, 20), (1, 36)])
def test_mixed_series_lengths_in_one_launch(I, H):
    """Series of 1, 2, 63, 64, 65 and 300 rows together; H = 64, the smallest H (4) and H = 20 / 36, which are no power of
    two and fill their register tile only in part; I = 1, 2, 3 (padded to 4 for the weight gradient) and 32."""
    from graphnet_amd import ops
    assert ops.gru_supported(I, H)
    xs, params, series_ptr, dout = _problem(I, H, LENGTHS)
    want, gru = R.gru_reference(xs, series_ptr, params)
    (want * dout.double()).sum().backward()
    out, grads = _device_pass(xs, params, series_ptr, dout)
    assert out.shape == (len(LENGTHS), H)
    print(f"I={I} H={H}: forward {rel_err(out, want.detach()):.2e}")
    assert rel_err(out, want.detach()) < 1e-4
    for name, p in gru.named_parameters():
        assert grads[name].shape == p.shape, name
        print(f"I={I} H={H}: grad {name} {rel_err(grads[name], p.grad):.2e}")
        assert rel_err(grads[name], p.grad) < 2e-3, name


def test_a_single_series_and_inference_without_saved_state():
    from graphnet_amd import ops
    for lengths in ([1], [5]):
        xs, params, series_ptr, dout = _problem(2, 64, lengths, seed=3)
        want, gru = R.gru_reference(xs, series_ptr, params)
        (want * dout.double()).sum().backward()
        out, grads = _device_pass(xs, params, series_ptr, dout)
        assert rel_err(out, want.detach()) < 1e-4
        for name, p in gru.named_parameters():
            assert rel_err(grads[name], p.grad) < 2e-3, name
        p = [params[k].to(DEV) for k in NAMES]
        out2, saved = ops.gru_series_fwd(xs.to(DEV), torch.from_numpy(series_ptr).to(DEV), *p, save=False)
        assert saved is None and torch.equal(out2, out)


def test_two_runs_agree_bit_for_bit():
    lengths = LENGTHS * 40 + [1] * 3000                            # more series than resident waves take in one round
    xs, params, series_ptr, dout = _problem(2, 64, lengths, seed=7)
    out1, g1 = _device_pass(xs, params, series_ptr, dout)
    out2, g2 = _device_pass(xs, params, series_ptr, dout)
    assert torch.equal(out1, out2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    want, _ = R.gru_reference(xs, series_ptr, params)
    assert rel_err(out1, want.detach()) < 1e-4


def test_outside_the_envelope_raises():
    import graphnet_amd as g
    from graphnet_amd import ops
    assert not ops.gru_supported(2, 128) and not ops.gru_supported(33, 64) and not ops.gru_supported(2, 66)
    xs, params, series_ptr, dout = _problem(2, 128, [3, 2])
    with pytest.raises(RuntimeError, match="envelope"):
        ops.gru_series_fwd(xs.to(DEV), torch.from_numpy(series_ptr).to(DEV), *[params[k].to(DEV) for k in NAMES])
    m = g.Node_RNN(2, 128, 1, [4, 3]).to(DEV)
    b = g.Batch(x=torch.rand(5, 6, device=DEV), n_pulses=torch.tensor([5], dtype=torch.int32, device=DEV),
                batch=torch.zeros(5, dtype=torch.int64, device=DEV))
    b.x[:, 5] = torch.tensor([1.0, 0, 0, 1, 0], device=DEV)
    with pytest.raises(RuntimeError, match="no torch fallback"):
        m(b)


def _series_rows(seed=2):
    """Rows as NodeAsDOMTimeSeries writes them: x, y, z, t, charge, new_node_col; three events."""
    rng = np.random.default_rng(seed)
    lengths = [3, 1, 1, 70, 2, 1, 9, 1]
    per_event = [3, 2, 3]
    rows = rng.normal(size=(sum(lengths), 6)).astype(np.float32)
    rows[:, 4] = rng.uniform(0.1, 4.0, size=len(rows)).astype(np.float32)
    series_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rows[:, 5] = 0
    rows[series_ptr[:-1], 5] = 1
    dom_ptr = np.concatenate([[0], np.cumsum(per_event)]).astype(np.int32)
    batch = np.repeat(np.arange(3), [series_ptr[dom_ptr[e + 1]] - series_ptr[dom_ptr[e]] for e in range(3)])
    return rows, series_ptr, dom_ptr, batch


@pytest.mark.parametrize("embedding_dim", [0, 16])
def test_node_rnn_computes_layer_0_only(embedding_dim):
    """``num_layers = 2``: the output is the reference's ``[-1][0]`` (layer 0's final state), the layer-1 parameters get no
    gradient.  With and without the batch's ``series_ptr`` / ``dom_ptr``; with the sinusoidal embedding (I = 32)."""
    import graphnet_amd as g
    rows, series_ptr, dom_ptr, batch = _series_rows()
    torch.manual_seed(3)
    m = g.Node_RNN(2, 64, 2, [4, 3], embedding_dim=embedding_dim).to(DEV)
    b = g.Batch(x=torch.from_numpy(rows).to(DEV), batch=torch.from_numpy(batch).to(DEV),
                n_pulses=torch.tensor([5, 72, 11], dtype=torch.int32, device=DEV))
    out = m(b)                                                      # series derived from new_node_col and batch
    assert "edge_index" not in out.keys() and out.n_pulses.tolist() == [5, 72, 11]
    assert out.ptr.tolist() == dom_ptr.tolist() and out.batch.tolist() == np.repeat(np.arange(3), np.diff(dom_ptr)).tolist()
    b.series_ptr, b.dom_ptr = torch.from_numpy(series_ptr).to(DEV), torch.from_numpy(dom_ptr).to(DEV)
    out2 = m(b)
    assert torch.equal(out.x, out2.x) and torch.equal(out.ptr, out2.ptr) and torch.equal(out.batch, out2.batch)
    w = torch.randn(out.x.shape, generator=torch.Generator().manual_seed(1))
    (out2.x * w.to(DEV)).sum().backward()
    # the reference's lines: the embedding in fp32 as its module computes it (components/embedding.py:42-50; the arguments
    # reach ~10^4 rad, so the fp32 products ARE the definition), the GRU in float64
    ts = torch.from_numpy(rows[:, [4, 3]])
    if embedding_dim:
        half_dim = embedding_dim / 2
        emb = torch.log(torch.Tensor([10000])) / half_dim
        emb = torch.exp(torch.arange(half_dim) * (-emb))
        emb = (ts * 4096).unsqueeze(-1) * emb.unsqueeze(0)
        ts = torch.cat((torch.sin(emb), torch.cos(emb)), dim=-1).reshape((len(rows), embedding_dim * 2))
    params = {k: v.detach().cpu() for k, v in m._rnn.named_parameters()}
    want, gru = R.gru_reference(ts, series_ptr, params, num_layers=2)
    (want * w[:, 5:].double()).sum().backward()
    assert out.x.shape == (8, 69)
    assert rel_err(out.x[:, 5:], want.detach()) < 1e-4
    assert rel_err(out.x[:, :5], R.dom_rows_reference(rows, series_ptr, 4)) < 1e-6
    for name, p in m._rnn.named_parameters():
        ref_grad = gru.get_parameter(name).grad
        if name.endswith("_l1"):
            assert p.grad is None and (ref_grad is None or not bool(ref_grad.any())), name
        else:
            assert rel_err(p.grad, ref_grad) < 2e-3, name


def test_dom_series_summary_rows_and_asinh_of_the_summed_charge():
    from graphnet_amd import ops
    rng = np.random.default_rng(9)
    lengths = [1, 2, 63, 64, 65, 300, 1] * 40
    rows = rng.normal(size=(sum(lengths), 7)).astype(np.float32)
    rows[:, 2] = rng.uniform(0.0, 30.0, size=len(rows)).astype(np.float32)
    series_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    got = ops.dom_series_summary(torch.from_numpy(rows).to(DEV), torch.from_numpy(series_ptr).to(DEV), 6, 2)
    want = R.dom_rows_reference(rows, series_ptr, 2)
    assert got.shape == (len(lengths), 6)
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(got.cpu().numpy()[:, keep], want[:, keep].astype(np.float32))
    # one fp32 sum of up to 300 non-negative terms and one asinh, whose slope 1 / sqrt(1 + s^2) turns the sum's relative
    # error into an absolute one; relative to the largest entry (asinh(4500) = 9.1)
    assert rel_err(got[:, 2], want[:, 2]) < 1e-6
