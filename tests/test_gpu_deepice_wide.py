"""GPU tests of ``graphnet_amd.DeepIce`` with ``head_size=64`` (the biased blocks on ``csrc/attn_rel_wide.hip``) against the
float64 restatement of ``tests/deepice_reference.py``: forward and every parameter gradient.  Pulses, helpers and gates are
those of ``test_gpu_deepice.py``: fp32 1e-4 forward and 2e-3 gradients, bf16 2e-2 forward and the Frobenius bound."""
import functools

import pytest
import torch

import deepice_reference as ref
from test_gpu_deepice import DEV, SIZES, _batch, _ours, _pulses
from test_gpu_tito import BF16_GRAD_FROBENIUS, norm_err, rel_err

pytestmark = pytest.mark.gpu
BASE = dict(hidden_dim=128, head_size=64, seq_length=32, depth=2, depth_rel=2)


@functools.lru_cache(maxsize=None)
def _models(n_rel):
    """The restatement in float64 with its weights moved off their initial values, shared by the two modes."""
    kw = dict(BASE, n_rel=n_rel)
    torch.manual_seed(64 + n_rel)
    theirs = ref.DeepIce(**kw).double()
    with torch.no_grad():
        for name, p in theirs.named_parameters():
            if "gamma" in name or "norm" in name or name.endswith(".1.weight") or name.endswith(".1.bias"):
                p.add_(0.2 * torch.randn_like(p))
    return kw, theirs


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("n_rel", [1, 2])
def test_forward_and_parameter_gradients(n_rel, mode):
    kw, theirs = _models(n_rel)
    m = _ours(kw, theirs, mode)
    x, batch = _pulses()
    b = _batch(x, batch)
    y = m(b.to(DEV))
    assert y.shape == (len(SIZES), kw["hidden_dim"]) and y.dtype == torch.float32
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    theirs.zero_grad(set_to_none=True)
    yo = theirs(b.x.cpu(), batch, None, None)
    (yo * w.double()).sum().backward()
    e = rel_err(y, yo.detach())
    print(f"DeepIce head_size=64 n_rel={n_rel} {mode} forward: {e:.3e}")
    assert e < (1e-4 if mode == "fp32" else 2e-2)
    po_all = dict(theirs.named_parameters())
    errs = {}
    for kn, p in m.named_parameters():
        po = po_all[kn]
        if po.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, kn
            continue
        assert p.grad is not None, kn
        errs[kn] = rel_err(p.grad, po.grad) if mode == "fp32" else norm_err(p.grad, po.grad)
    worst = max(errs, key=errs.get)
    print(f"DeepIce head_size=64 n_rel={n_rel} {mode} worst gradient: {errs[worst]:.3e} ({worst})")
    bad = [(kn, ge) for kn, ge in errs.items() if not ge < (2e-3 if mode == "fp32" else BF16_GRAD_FROBENIUS)]
    assert not bad, bad
