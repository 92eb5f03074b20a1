"""GPU tests of the biased ragged attention at head width 64 with ``s_ij`` formed once per pair for a group of 4 heads
(``gn_rel_attention_wide_shared_fwd`` / ``_bwd``, ``csrc/attn_rel_wide_shared.hip``) against the attention core of
``tests/deepice_reference.py`` in float64 and, bit for bit, against the two-lane kernels of ``csrc/attn_rel_wide.hip``.
Inputs, restatement, gates and ``rel_err`` are those of ``test_gpu_rel_attention.py``, the event sizes those of
``test_gpu_rel_attention_wide.py`` (rows on each side of the boundary between the two waves of a pair, tile tails, a
multi-tile event, a single-key softmax; 2, 31, 33, 65 and 130 end in a partly filled block of 4 rows).

Heads: 1 and 3 leave wave pairs of the workgroup without a head (they still form their share of ``s_ij``), 9 needs a third
head group that holds one head."""
import pytest
import torch

from test_gpu_rel_attention import FLOOR, FWD_GATE, GRAD_GATE, _case, _inputs
from test_gpu_rel_attention_wide import SIZES
from test_gpu_tito import rel_err

pytestmark = pytest.mark.gpu


def _run(c, H, family="rel_attention_wide_shared"):
    from graphnet_amd import ops
    dev, dh = "cuda", 64
    xt, qkv, qp, ptr = c["xt"].to(dev), c["qkv"].to(dev), c["qp"].to(dev), c["ptr"].to(dev)
    freq = ops.rel_attention_freq(dh, dev)
    plan = ops.attention_plan(ptr)
    out, u, lse2 = getattr(ops, family + "_fwd")(qkv, qp, xt, freq, H, ptr, plan)
    dqkv, dqp = getattr(ops, family + "_bwd")(qkv, qp, xt, freq, H, ptr, plan, out, u, lse2, c["dout"].to(dev), c["du"].to(dev))
    torch.cuda.synchronize()
    d = H * dh
    return dict(out=out, u=u, dq=dqkv[:, :d], dk=dqkv[:, d:2 * d], dv=dqkv[:, 2 * d:], dqp=dqp, lse2=lse2, dqkv=dqkv)


@pytest.mark.parametrize("H", [1, 3, 9])
def test_forward_and_gradients_against_the_float64_restatement(H):
    from graphnet_amd import ops
    assert ops.rel_attention_wide_shared_supported(64)
    c = _case(H, 64, SIZES)
    got = _run(c, H)
    bad = []
    for name in ("out", "u", "dq", "dk", "dv", "dqp"):
        e32 = rel_err(c["ref32"][name], c["ref64"][name])
        e = rel_err(got[name], c["ref64"][name])
        gate = min(max(4.0 * e32, FLOOR), FWD_GATE if name in ("out", "u") else GRAD_GATE)
        print(f"rel_attention_wide_shared H={H} {name}: kernel {e:.3e}  fp32 restatement {e32:.3e}  gate {gate:.3e}")
        if not e <= gate:
            bad.append((name, e, gate))
    assert not bad, bad
    # the event of one pulse: a softmax over one key has no gradient w.r.t. its score
    d = H * 64
    assert torch.count_nonzero(got["dq"][0]) == 0 and torch.count_nonzero(got["dk"][0]) == 0 and torch.count_nonzero(got["dqp"][0]) == 0
    assert torch.equal(got["out"][0].cpu(), c["qkv"][0, 2 * d:])


@pytest.mark.parametrize("H", [1, 3, 9])
def test_the_same_bits_as_the_two_lane_kernels(H):
    c = _case(H, 64, SIZES)
    got, two_lane = _run(c, H), _run(c, H, "rel_attention_wide")
    for name in ("out", "u", "lse2", "dqkv", "dqp"):
        assert torch.equal(got[name], two_lane[name]), name


def test_two_runs_agree_bit_for_bit():
    """More workgroups than the device keeps resident (2 to 3 tiles x 3 head groups x 500 events)."""
    H = 9
    c = _inputs(H, 64, [70, 65, 90, 128, 129] * 100)
    a, b = _run(c, H), _run(c, H)
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert bool(torch.isfinite(a[name]).all()), name


def test_deepice_with_shared_bias(monkeypatch):
    """The small ``DeepIce`` of ``test_gpu_deepice_wide.py`` (head size 64, fp32 mode, its gates) with
    ``Attention_rel.shared_bias``."""
    import graphnet_amd as g
    from test_gpu_deepice import DEV, SIZES as EVENTS, _batch, _ours, _pulses
    from test_gpu_deepice_wide import _models
    monkeypatch.setattr(g.Attention_rel, "shared_bias", True)            # restored when the test ends
    kw, theirs = _models(2)
    m = _ours(kw, theirs, "fp32")
    x, batch = _pulses()
    b = _batch(x, batch)
    y = m(b.to(DEV))
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    theirs.zero_grad(set_to_none=True)
    yo = theirs(b.x.cpu(), batch, None, None)
    (yo * w.double()).sum().backward()
    assert y.shape == (len(EVENTS), kw["hidden_dim"]) and rel_err(y.detach(), yo.detach()) < 1e-4
    po_all = dict(theirs.named_parameters())
    bad = [(kn, rel_err(p.grad, po_all[kn].grad)) for kn, p in m.named_parameters()
           if po_all[kn].grad is not None and not rel_err(p.grad, po_all[kn].grad) < 2e-3]
    assert not bad, bad


@pytest.mark.parametrize("dh", [16, 32])
def test_unsupported_head_width_raises(dh):
    from graphnet_amd import ops
    assert not ops.rel_attention_wide_shared_supported(dh)
    N, H = 8, 2
    qkv, qp, xt = torch.zeros(N, 3 * H * dh, device="cuda"), torch.zeros(N, H * dh, device="cuda"), torch.zeros(N, 4, device="cuda")
    ptr = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError, match="head width"):
        ops.rel_attention_wide_shared_fwd(qkv, qp, xt, ops.rel_attention_freq(dh, "cuda"), H, ptr, ops.attention_plan(ptr))
