"""GPU tests of the ragged attention with the on-the-fly spacetime bias (``gn_rel_attention_fwd`` / ``_bwd``,
``csrc/attn_rel.hip``) against the attention core of ``tests/deepice_reference.py`` in float64.

Gate: the kernel's error is at most 4x the error of the SAME restatement evaluated in fp32 on the same inputs (the factor
covers the different summation order and sine implementation), with a floor of 1e-5, and never above the project's fp32
gates (1e-4 forward, 2e-3 gradients).  Errors are ``max|a - b| / max|b|`` per tensor (``rel_err`` of ``test_gpu_tito.py``)."""
import functools

import pytest
import torch

import deepice_reference as ref
from test_gpu_tito import rel_err

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 130, 200]          # tile tails, a single-key softmax, multi-tile events
FWD_GATE, GRAD_GATE, FLOOR = 1e-4, 2e-3, 1e-5


def _pulses(sizes, seed):
    """fp32 ``[N, 4]`` (x, y, z, time), standardised ranges.  The second half of the 65- and 200-pulse events sits on one
    DOM position (``ds < 0`` off the diagonal, 0 on it); three pulses of the largest event are so far apart in time that
    the clip at +-4 acts on all their pairs."""
    gen = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    xt = torch.cat([torch.rand(N, 3, generator=gen) * 2.4 - 1.2, torch.rand(N, 1, generator=gen) * 0.9 - 0.3], 1)
    off = 0
    for n in sizes:
        if n in (65, 200):
            xt[off + n // 2: off + n, :3] = xt[off + n // 2 - 1, :3]
        if n == max(sizes) and n >= 3:
            xt[off + 1, 3], xt[off + 2, 3], xt[off + n - 1, 3] = 10.0, -10.0, 30.0
        off += n
    return xt


def _inputs(H, dh, sizes):
    gen = torch.Generator().manual_seed(100 * H + dh)
    N, d = sum(sizes), H * dh
    ptr = torch.tensor([0] + list(sizes)).cumsum(0).to(torch.int32)
    return dict(xt=_pulses(sizes, seed=7), qkv=torch.randn(N, 3 * d, generator=gen), qp=torch.randn(N, d, generator=gen) * 0.5,
                dout=torch.randn(N, d, generator=gen), du=torch.randn(N, d, generator=gen), ptr=ptr)


@functools.lru_cache(maxsize=None)
def _case(H, dh, sizes=tuple(SIZES)):
    """Inputs and the restatement's results, float64 and fp32, computed once per shape and shared (read only)."""
    c = _inputs(H, dh, sizes)
    xt, qkv, qp, dout, du = c["xt"], c["qkv"], c["qp"], c["dout"], c["du"]
    d = H * dh
    res = {}
    for dtype in (torch.float64, torch.float32):
        a_qkv, a_qp = qkv.to(dtype).requires_grad_(), qp.to(dtype).requires_grad_()
        outs, us, off = [], [], 0
        for n in sizes:
            rows = slice(off, off + n)
            s = ref.sin_emb(ref.pair_argument(xt[rows]).to(dtype), dh)
            O, U = ref.attention_core(a_qkv[rows, :d], a_qkv[rows, d:2 * d], a_qkv[rows, 2 * d:], a_qp[rows], s, H)
            outs.append(O); us.append(U)
            off += n
        out, u = torch.cat(outs), torch.cat(us)
        ((out * dout.to(dtype)).sum() + (u * du.to(dtype)).sum()).backward()
        res[dtype] = dict(out=out.detach(), u=u.detach(), dq=a_qkv.grad[:, :d], dk=a_qkv.grad[:, d:2 * d], dv=a_qkv.grad[:, 2 * d:],
                          dqp=a_qp.grad)
    return dict(c, ref64=res[torch.float64], ref32=res[torch.float32])


def _run(c, H, dh):
    from graphnet_amd import ops
    dev = "cuda"
    xt, qkv, qp, ptr = c["xt"].to(dev), c["qkv"].to(dev), c["qp"].to(dev), c["ptr"].to(dev)
    freq = ops.rel_attention_freq(dh, dev)
    plan = ops.attention_plan(ptr)
    out, u, lse2 = ops.rel_attention_fwd(qkv, qp, xt, freq, H, ptr, plan)
    dqkv, dqp = ops.rel_attention_bwd(qkv, qp, xt, freq, H, ptr, plan, out, u, lse2, c["dout"].to(dev), c["du"].to(dev))
    torch.cuda.synchronize()
    d = H * dh
    return dict(out=out, u=u, dq=dqkv[:, :d], dk=dqkv[:, d:2 * d], dv=dqkv[:, 2 * d:], dqp=dqp, lse2=lse2)


SHAPES = [(3, 32), (1, 32)]


@pytest.mark.parametrize("H,dh", SHAPES)
def test_forward_and_gradients_against_the_float64_restatement(H, dh):
    from graphnet_amd import ops
    assert torch.equal(ops.rel_attention_freq(dh, "cpu"), ref.frequencies(dh))
    c = _case(H, dh)
    got = _run(c, H, dh)
    bad = []
    for name in ("out", "u", "dq", "dk", "dv", "dqp"):
        e32 = rel_err(c["ref32"][name], c["ref64"][name])
        e = rel_err(got[name], c["ref64"][name])
        gate = min(max(4.0 * e32, FLOOR), FWD_GATE if name in ("out", "u") else GRAD_GATE)
        print(f"rel_attention H={H} dh={dh} {name}: kernel {e:.3e}  fp32 restatement {e32:.3e}  gate {gate:.3e}")
        if not e <= gate:
            bad.append((name, e, gate))
    assert not bad, bad
    # the event of one pulse: a softmax over one key has no gradient w.r.t. its score
    d = H * dh
    assert torch.count_nonzero(c["ref64"]["dq"][0]) == 0 and torch.count_nonzero(c["ref64"]["dk"][0]) == 0
    assert torch.count_nonzero(got["dq"][0]) == 0 and torch.count_nonzero(got["dk"][0]) == 0 and torch.count_nonzero(got["dqp"][0]) == 0
    assert torch.equal(got["out"][0].cpu(), c["qkv"][0, 2 * d:])


def test_two_runs_agree_bit_for_bit():
    """More waves than the device keeps resident (2 tiles x 3 heads x 500 events), so that the order in which tiles
    start differs between runs."""
    H, dh = 3, 32
    c = _inputs(H, dh, [70, 65, 90, 128, 129] * 100)
    a, b = _run(c, H, dh), _run(c, H, dh)
    for name in a:
        assert torch.equal(a[name], b[name]), name
    assert bool(torch.isfinite(a["out"]).all()) and bool(torch.isfinite(a["dqp"]).all())


def test_without_bias_it_is_the_plain_ragged_attention():
    """``qp = 0`` and ``du = 0``: ``out``, ``lse2`` and ``dqkv`` equal ``ops.attention_fwd`` / ``attention_bwd`` (fp32)."""
    from graphnet_amd import ops
    H, dh = 3, 32
    c = dict(_case(H, dh))
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
        print(f"rel_attention without bias vs attention {name}: {e:.3e}")
        assert e < 1e-6, (name, e)
    assert bool(torch.isfinite(got["dqp"]).all())


def test_unsupported_head_width_raises():
    from graphnet_amd import ops
    assert ops.rel_attention_supported(32) and not ops.rel_attention_supported(16) and not ops.rel_attention_supported(64)
    for dh in (16, 64):
        N, H = 8, 2
        qkv = torch.zeros(N, 3 * H * dh, device="cuda")
        qp = torch.zeros(N, H * dh, device="cuda")
        xt = torch.zeros(N, 4, device="cuda")
        ptr = torch.tensor([0, N], dtype=torch.int32, device="cuda")
        with pytest.raises(NotImplementedError, match="head width"):
            ops.rel_attention_fwd(qkv, qp, xt, ops.rel_attention_freq(dh, "cuda"), H, ptr, ops.attention_plan(ptr))
