"""GPU tests of the biased ragged attention at head width 64 (``gn_rel_attention_wide_fwd`` / ``_bwd``,
``csrc/attn_rel_wide.hip``: two lanes per query) against the attention core of ``tests/deepice_reference.py`` in float64.
Inputs, restatement, gates and ``rel_err`` are those of ``test_gpu_rel_attention.py``.

The event sizes put a row on each side of the boundary between the two waves of a tile (31, 32, 33), a tile tail (65), a
multi-tile event (130), a single-key softmax (1), the same-DOM half of the 65-pulse event and the clipped pairs of the
largest one.  The restatement's own fp32 error on these inputs is 3.4e-5 to 1.0e-4 forward and 2.1e-5 to 6.5e-5 on the
gradients, which puts the gates at 1e-4 forward and 8e-5 to 2.6e-4 on the gradients."""
import pytest
import torch

from test_gpu_rel_attention import FLOOR, FWD_GATE, GRAD_GATE, _case, _inputs
from test_gpu_tito import rel_err

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 31, 32, 33, 64, 65, 130)


def _run(c, H, dh):
    from graphnet_amd import ops
    dev = "cuda"
    xt, qkv, qp, ptr = c["xt"].to(dev), c["qkv"].to(dev), c["qp"].to(dev), c["ptr"].to(dev)
    freq = ops.rel_attention_freq(dh, dev)
    plan = ops.attention_plan(ptr)
    out, u, lse2 = ops.rel_attention_wide_fwd(qkv, qp, xt, freq, H, ptr, plan)
    dqkv, dqp = ops.rel_attention_wide_bwd(qkv, qp, xt, freq, H, ptr, plan, out, u, lse2, c["dout"].to(dev), c["du"].to(dev))
    torch.cuda.synchronize()
    d = H * dh
    return dict(out=out, u=u, dq=dqkv[:, :d], dk=dqkv[:, d:2 * d], dv=dqkv[:, 2 * d:], dqp=dqp, lse2=lse2)


@pytest.mark.parametrize("H,dh", [(2, 64), (1, 64)])
def test_forward_and_gradients_against_the_float64_restatement(H, dh):
    from graphnet_amd import ops
    assert ops.rel_attention_wide_supported(dh) and not ops.rel_attention_wide_supported(32)
    c = _case(H, dh, SIZES)
    got = _run(c, H, dh)
    bad = []
    for name in ("out", "u", "dq", "dk", "dv", "dqp"):
        e32 = rel_err(c["ref32"][name], c["ref64"][name])
        e = rel_err(got[name], c["ref64"][name])
        gate = min(max(4.0 * e32, FLOOR), FWD_GATE if name in ("out", "u") else GRAD_GATE)
        print(f"rel_attention_wide H={H} dh={dh} {name}: kernel {e:.3e}  fp32 restatement {e32:.3e}  gate {gate:.3e}")
        if not e <= gate:
            bad.append((name, e, gate))
    assert not bad, bad
    # the event of one pulse: a softmax over one key has no gradient w.r.t. its score
    d = H * dh
    assert torch.count_nonzero(c["ref64"]["dq"][0]) == 0 and torch.count_nonzero(c["ref64"]["dk"][0]) == 0
    assert torch.count_nonzero(got["dq"][0]) == 0 and torch.count_nonzero(got["dk"][0]) == 0 and torch.count_nonzero(got["dqp"][0]) == 0
    assert torch.equal(got["out"][0].cpu(), c["qkv"][0, 2 * d:])


def test_two_runs_agree_bit_for_bit():
    """More workgroups than the device keeps resident (2 to 3 tiles x 2 heads x 500 events)."""
    H, dh = 2, 64
    c = _inputs(H, dh, [70, 65, 90, 128, 129] * 100)
    a, b = _run(c, H, dh), _run(c, H, dh)
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert bool(torch.isfinite(a[name]).all()), name


def test_without_bias_it_is_the_plain_ragged_attention():
    """``qp = 0`` and ``du = 0``: ``out``, ``lse2`` and ``dqkv`` equal ``ops.attention_fwd`` / ``attention_bwd`` (fp32)."""
    from graphnet_amd import ops
    H, dh = 2, 64
    c = dict(_case(H, dh, SIZES))
    c["qp"], c["du"] = torch.zeros_like(c["qp"]), torch.zeros_like(c["du"])
    got = _run(c, H, dh)
    qkv, ptr = c["qkv"].to("cuda"), c["ptr"].to("cuda")
    plan = ops.attention_plan(ptr)
    out, lse2 = ops.attention_fwd(qkv, H, ptr, plan)
    dqkv = ops.attention_bwd(qkv, H, ptr, plan, out, lse2, c["dout"].to("cuda"))
    d = H * dh
    for name, a, b in (("out", got["out"], out), ("lse2", got["lse2"], lse2), ("dq", got["dq"], dqkv[:, :d]),
                       ("dk", got["dk"], dqkv[:, d:2 * d]), ("dv", got["dv"], dqkv[:, 2 * d:])):
        e = rel_err(a, b)
        print(f"rel_attention_wide without bias vs attention {name}: {e:.3e}")
        assert e < 1e-6, (name, e)
