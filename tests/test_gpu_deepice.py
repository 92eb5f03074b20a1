"""GPU tests of ``graphnet_amd.DeepIce`` against the float64 restatement of the reference's dense, padded formulation
(``tests/deepice_reference.py``): forward and every parameter gradient.

fp32 mode: 1e-4 forward, 2e-3 gradients (``max|a - b| / max|b|``).  bf16 mode: 2e-2 forward and the per-tensor Frobenius
bound of ``test_gpu_tito.py`` on gradients.  The embedded DynEdge rebuilds its graph from latent features; the graphs the
device built are handed to the restatement (teacher forcing), as ``test_dynedge_as_embedded_in_deepice`` does."""
import functools

import pytest
import torch

import deepice_reference as ref
from test_gpu_tito import BF16_GRAD_FROBENIUS, norm_err, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 2, 65, 130]
BASE = dict(hidden_dim=64, head_size=32, seq_length=32, depth=2, depth_rel=2)
DYNEDGE_ARGS = dict(nb_inputs=6, nb_neighbours=9, post_processing_layer_sizes=[48, 32], dynedge_layer_sizes=[(32, 48), (48, 32)],
                    global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)
CASES = {
    "n_rel1": dict(n_rel=1),
    "n_rel2": dict(n_rel=2),
    "n_rel0": dict(n_rel=0),                     # the reference's quirk: every sandwich block keeps the bias
    "features4": dict(n_rel=1, n_features=4),
    "scaled_emb": dict(n_rel=1, scaled_emb=True),
    "dynedge": dict(n_rel=1, include_dynedge=True, dynedge_args=DYNEDGE_ARGS),
}


def _pulses(sizes=SIZES, seed=11):
    """``[N, 6]`` fp32 in the standardised ranges of ``IceCubeKaggle``: x, y, z, time, charge, auxiliary in {0, 1}; the second
    half of the 65-pulse event sits on one DOM position."""
    gen = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    x = torch.cat([torch.rand(N, 3, generator=gen) * 2.0 - 1.0, torch.rand(N, 1, generator=gen) * 0.9 - 0.3,
                   torch.rand(N, 1, generator=gen) * 1.2 - 0.4, torch.randint(0, 2, (N, 1), generator=gen).float()], 1)
    off = 0
    for n in sizes:
        if n == 65:
            x[off + n // 2: off + n, :3] = x[off + n // 2 - 1, :3]
        off += n
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return x, batch


def _batch(x, batch):
    import graphnet_amd as g
    n = torch.bincount(batch)
    b = g.Batch(x=x.clone())
    b.batch = batch.clone()
    b.ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    b.n_pulses = n.to(torch.int32)
    return b


@functools.lru_cache(maxsize=None)
def _models(case):
    """The restatement in float64 with its weights (every case draws its own), shared by the tests of the case."""
    kw = dict(BASE, **CASES[case])
    torch.manual_seed(sum(map(ord, case)))
    theirs = ref.DeepIce(**kw).double()
    with torch.no_grad():                        # away from the initial values 1 and 0, so that every gradient is exercised
        for name, p in theirs.named_parameters():
            if "gamma" in name or "norm" in name or name.endswith(".1.weight") or name.endswith(".1.bias"):
                p.add_(0.2 * torch.randn_like(p))
    return kw, theirs


def _ours(kw, theirs, mode):
    import graphnet_amd as g
    m = g.DeepIce(**kw)
    m.load_state_dict({k: v.float() for k, v in theirs.state_dict().items()})
    return m.to(DEV).set_backend(dtype=mode)


def _forced_graphs(m, b, oracle):
    """(layer-1 graph from the oracle's k-NN on x, y, z, t, then the graphs the device DynEdge built)."""
    ei0 = oracle.knn_graph(b.x, 6, b.batch, [0, 1, 2, 3])
    b.edge_index = ei0
    bd = b.to(DEV)
    with torch.no_grad():
        _, trace = m.dyn_edge(bd, return_trace=True)
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], ei0)
    return bd, ei0, forced


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_parameter_gradients(oracle, case, mode):
    kw, theirs = _models(case)
    m = _ours(kw, theirs, mode)
    x, batch = _pulses()
    F = kw.get("n_features", 6)
    b = _batch(x[:, :max(F, 4)] if not kw.get("include_dynedge") else x, batch)
    ei0 = forced = None
    if kw.get("include_dynedge"):
        bd, ei0, forced = _forced_graphs(m, b, oracle)
    else:
        bd = b.to(DEV)
    y = m(bd)
    assert y.shape == (len(SIZES), kw["hidden_dim"]) and y.dtype == torch.float32
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    theirs.zero_grad(set_to_none=True)
    yo = theirs(b.x.cpu(), batch, ei0, forced)
    (yo * w.double()).sum().backward()
    e = rel_err(y, yo.detach())
    print(f"DeepIce {case} {mode} forward: {e:.3e}")
    assert e < (1e-4 if mode == "fp32" else 2e-2)
    bad = []
    po_all = dict(theirs.named_parameters())
    for kn, p in m.named_parameters():
        po = po_all[kn]
        if po.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, kn
            continue
        assert p.grad is not None, kn
        ge = rel_err(p.grad, po.grad) if mode == "fp32" else norm_err(p.grad, po.grad)
        if not ge < (2e-3 if mode == "fp32" else BF16_GRAD_FROBENIUS):
            bad.append((kn, ge))
    worst = max((rel_err(p.grad, po_all[kn].grad) if mode == "fp32" else norm_err(p.grad, po_all[kn].grad), kn)
                for kn, p in m.named_parameters() if po_all[kn].grad is not None)
    print(f"DeepIce {case} {mode} worst gradient: {worst[0]:.3e} ({worst[1]})")
    assert not bad, bad


def test_an_event_does_not_depend_on_the_rest_of_the_batch():
    """fp32 mode, 1e-5 of the output's maximum: the attention kernels give an event the same bits in any batch, the GEMMs of
    the device library may sum in another order when the row count changes."""
    kw, theirs = _models("n_rel1")
    m = _ours(kw, theirs, "fp32")
    x, batch = _pulses()
    with torch.no_grad():
        full = m(_batch(x, batch).to(DEV))
        for e in (0, 2):
            rows = batch == e
            alone = m(_batch(x[rows], torch.zeros(int(rows.sum()), dtype=torch.int64)).to(DEV))
            err = rel_err(alone[0], full[e])
            print(f"DeepIce event {e} alone vs in the batch: {err:.3e}")
            assert err < 1e-5


def test_a_standard_model_training_step_stays_finite():
    import graphnet_amd as g
    torch.manual_seed(5)
    model = g.StandardModel(
        graph_definition=g.KNNGraph(g.IceCubeKaggle(), input_feature_names=["x", "y", "z", "time", "charge", "auxiliary"]),
        backbone=g.DeepIce(n_rel=1, **BASE),
        tasks=[g.DirectionReconstructionWithKappa(hidden_size=BASE["hidden_dim"], target_labels="direction",
                                                  loss_function=g.VonMisesFisher3DLoss())],
        optimizer_class=torch.optim.AdamW, optimizer_kwargs=dict(lr=1e-3, eps=1e-7, weight_decay=0.05)).to(DEV)
    x, batch = _pulses()
    b = _batch(x, batch)
    b.direction = torch.nn.functional.normalize(torch.randn(len(SIZES), 3), dim=1)
    b = b.to(DEV)
    opt, _ = model.configure_optimizers()
    model.train()
    losses = []
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        loss = model.shared_step(b)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(torch.isfinite(torch.tensor(losses)))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.backbone.parameters())
