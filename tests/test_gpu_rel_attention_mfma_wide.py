"""GPU tests of the biased ragged attention at head width 64 with bf16 operands on the matrix cores
(``gn_rel_attention_mfma_wide_fwd`` / ``_bwd``, ``csrc/attn_rel_mfma_wide.hip``) against the attention core of
``tests/deepice_reference.py`` in float64.

``qkv``, ``qp``, ``dout`` and ``du`` are rounded to bf16 before both sides; the reference keeps ``s_ij`` unrounded.  Gate: the
project's gate of the bf16 matrix-core attention, ``rel_err < 2e-2`` per tensor (``test_gpu_tito.py``), as at head width 32."""
import pytest
import torch

import deepice_reference as ref
from test_gpu_rel_attention import SIZES, _inputs
from test_gpu_tito import rel_err

pytestmark = pytest.mark.gpu

G, DH, GATE = 16, 64, 2e-2                     # heads of a workgroup, head width
ROWS = ("qkv", "qp", "dout", "du")


def _case(H):
    """bf16-rounded inputs and the float64 restatement's results on them."""
    c = _inputs(H, DH, SIZES)
    c.update({k: c[k].to(torch.bfloat16) for k in ROWS})
    d = H * DH
    qkv, qp = c["qkv"].double().requires_grad_(), c["qp"].double().requires_grad_()
    outs, us, off = [], [], 0
    for n in SIZES:
        rows = slice(off, off + n)
        s = ref.sin_emb(ref.pair_argument(c["xt"][rows]).double(), DH)
        O, U = ref.attention_core(qkv[rows, :d], qkv[rows, d:2 * d], qkv[rows, 2 * d:], qp[rows], s, H)
        outs.append(O); us.append(U)
        off += n
    out, u = torch.cat(outs), torch.cat(us)
    ((out * c["dout"].double()).sum() + (u * c["du"].double()).sum()).backward()
    c["ref64"] = dict(out=out.detach(), u=u.detach(), dq=qkv.grad[:, :d], dk=qkv.grad[:, d:2 * d], dv=qkv.grad[:, 2 * d:], dqp=qp.grad)
    return c


def _run(c, H):
    from graphnet_amd import ops
    t = {k: c[k].to("cuda", torch.bfloat16) for k in ROWS}
    xt, ptr = c["xt"].to("cuda"), c["ptr"].to("cuda")
    freq, plan = ops.rel_attention_freq(DH, "cuda"), ops.attention_plan(ptr)
    out, u, lse2 = ops.rel_attention_mfma_wide_fwd(t["qkv"], t["qp"], xt, freq, H, ptr, plan)
    dqkv, dqp = ops.rel_attention_mfma_wide_bwd(t["qkv"], t["qp"], xt, freq, H, ptr, plan, out, u, lse2, t["dout"], t["du"])
    torch.cuda.synchronize()
    d = H * DH
    return dict(out=out, u=u, dq=dqkv[:, :d], dk=dqkv[:, d:2 * d], dv=dqkv[:, 2 * d:], dqp=dqp, lse2=lse2)


@pytest.mark.parametrize("H", [1, 3, G + 1])       # waves without a head; a second group that holds one head
def test_forward_and_gradients_against_the_float64_restatement(H):
    c = _case(H)
    got = _run(c, H)
    errs = {name: rel_err(got[name].float(), c["ref64"][name]) for name in ("out", "u", "dq", "dk", "dv", "dqp")}
    print(f"rel_attention_mfma_wide H={H}: " + "  ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert all(e < GATE for e in errs.values()), errs
    assert got["out"].dtype == torch.bfloat16 and got["dqp"].dtype == torch.bfloat16 and got["lse2"].dtype == torch.float32
    assert torch.equal(got["out"][0].cpu(), c["qkv"][0, 2 * H * DH:])             # the event of one pulse: out = v


def test_two_runs_agree_bit_for_bit():
    H = G + 1
    c = _inputs(H, DH, [70, 65, 90, 128, 129] * 100)
    a, b = _run(c, H), _run(c, H)
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert bool(torch.isfinite(a[name].float()).all()), name


def test_deepice_with_matrix_bias(monkeypatch):
    """The small ``DeepIce`` of ``test_gpu_deepice_wide.py`` (``head_size=64``, bf16 mode, its gates) with
    ``Attention_rel.matrix_bias``."""
    import graphnet_amd as g
    from graphnet_amd import ops
    from test_gpu_deepice import DEV, SIZES as EVENTS, _batch, _ours, _pulses
    from test_gpu_deepice_wide import BF16_GRAD_FROBENIUS, _models, norm_err
    monkeypatch.setattr(g.Attention_rel, "matrix_bias", True)            # restored when the test ends
    kw, theirs = _models(2)
    m = _ours(kw, theirs, "bf16")
    x, batch = _pulses()
    b = _batch(x, batch)
    ops.enable_timers(True)
    y = m(b.to(DEV))
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    launched = ops.timer_summary()
    ops.enable_timers(False)
    theirs.zero_grad(set_to_none=True)
    yo = theirs(b.x.cpu(), batch, None, None)
    (yo * w.double()).sum().backward()
    assert "rel_attention_mfma_wide_fwd" in launched and "rel_attention_mfma_wide_bwd" in launched
    assert "rel_attention_wide_fwd" not in launched
    e = rel_err(y.detach(), yo.detach())
    po_all = dict(theirs.named_parameters())
    grads = {kn: norm_err(p.grad, po_all[kn].grad) for kn, p in m.named_parameters() if po_all[kn].grad is not None}
    worst = max(grads, key=grads.get)
    print(f"DeepIce head_size=64 n_rel=2 bf16 matrix_bias forward: {e:.3e}  worst gradient: {grads[worst]:.3e} ({worst})")
    assert y.shape == (len(EVENTS), kw["hidden_dim"]) and e < 2e-2
    bad = {kn: ge for kn, ge in grads.items() if not ge < BF16_GRAD_FROBENIUS}
    assert not bad, bad


@pytest.mark.parametrize("dh,dtype", [(16, torch.bfloat16), (32, torch.bfloat16), (64, torch.float32)])
def test_unsupported_head_width_and_wrong_dtype_raise(dh, dtype):
    from graphnet_amd import ops
    assert ops.rel_attention_mfma_wide_supported(64) and not ops.rel_attention_mfma_wide_supported(dh if dh != 64 else 32)
    N, H = 8, 2
    qkv, qp = torch.zeros(N, 3 * H * dh, device="cuda", dtype=dtype), torch.zeros(N, H * dh, device="cuda", dtype=dtype)
    xt, ptr = torch.zeros(N, 4, device="cuda"), torch.tensor([0, N], dtype=torch.int32, device="cuda")
    args = (qkv, qp, xt, ops.rel_attention_freq(dh, "cuda"), H, ptr, ops.attention_plan(ptr))
    if dtype == torch.float32:
        with pytest.raises(TypeError, match="qkv"):
            ops.rel_attention_mfma_wide_fwd(*args)
    else:
        with pytest.raises(NotImplementedError, match="head width"):
            ops.rel_attention_mfma_wide_fwd(*args)
