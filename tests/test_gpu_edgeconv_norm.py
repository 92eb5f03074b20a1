"""GPU: the fused LayerNorm + GELU edge kernels (``csrc/edgeconv_norm.hip``: ``ops.edgeconv_norm_fwd / _bwd``,
``DynEdge.set_backend(fused_norm_edge=True)``) against a plain float64 torch restatement (gather, layer_norm, gelu, matmul,
layer_norm, gelu, index_add; autograd for the gradients).

Gate: on the same inputs the unfused path (``csrc/generic.hip``, what ``fused_norm_edge=False`` runs) is measured against the
same float64 reference, and the fused path may have at most TWICE that error per compared tensor (fp32 mode: max-abs error over
the reference's max-abs; bf16 mode: Frobenius-relative error).

Measured on an MI355X, kernel test at (H1, H2) = (336, 256), k = 9, error against float64 (unfused / fused):

    tensor   fp32 mode (max-abs / max-abs)   bf16 mode (Frobenius-relative)
    out      2.65e-07 / 2.65e-07             2.03e-03 / 1.61e-03
    dP       2.93e-07 / 2.93e-07             2.97e-03 / 2.71e-03
    dQ       3.98e-07 / 4.11e-07             4.53e-03 / 3.84e-03
    dW2      4.46e-07 / 4.46e-07             2.03e-03 / 1.65e-03
    db2      7.79e-08 / 7.79e-08             1.53e-03 / 1.33e-03
    dgamma1  1.79e-07 / 1.84e-07             2.83e-03 / 2.37e-03
    dbeta1   2.39e-07 / 2.20e-07             2.56e-03 / 2.25e-03
    dgamma2  1.01e-07 / 7.79e-08             1.74e-03 / 1.41e-03
    dbeta2   7.07e-08 / 7.49e-08             1.26e-03 / 1.07e-03

Model test, worst tensor: fp32 1.90e-06 / 1.98e-06, bf16 9.5e-03 / 9.2e-03; largest fused / unfused ratio of any compared
tensor in the file: 1.42."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = [("fp32", 0), ("bf16", 1)]
# a single pulse (no edge), fewer pulses than k, four ordinary events: 150 pulses.  With an overflow edge on every third full
# centre the k = 8 plan has a tile of exactly 64 rows and the k = 9 plan closes tiles in the middle at 55 to 58 rows.
EVENTS = [1, 6, 40, 30, 50, 23]


def err(mode, a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double()
    if mode == 0:
        return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def gate(name, e_fused, e_unfused):
    print(f"{name}: unfused {e_unfused:.3e} fused {e_fused:.3e}")
    assert e_fused <= 2.0 * e_unfused, (name, e_fused, e_unfused)


def table(k):
    """Host-built neighbour table of EVENTS: centre i takes the next min(k, n - 1) pulses of its event (cyclically); every
    third centre with a full table also gets an overflow edge (k + 1 rows)."""
    from graphnet_amd import ops
    N = sum(EVENTS)
    nbr = torch.full((N, k), -1, dtype=torch.int32)
    ovf = torch.full((N,), -1, dtype=torch.int32)
    first = 0
    for n in EVENTS:
        for a in range(n):
            deg = min(k, n - 1)
            nbr[first + a, :deg] = first + (a + 1 + torch.arange(deg)) % n
            if deg == k and n - 1 > k and a % 3 == 0:
                ovf[first + a] = first + (a + 1 + k) % n
        first += n
    return ops._finish_table(nbr.to(DEV), ovf.to(DEV), k)


def kernel_case(mode, H1, H2, k):
    from graphnet_amd import ops
    H1p = ops.round_up(H1, 32)
    g = table(k)
    N = g.N
    gen = torch.Generator().manual_seed(100 * H1 + k)
    rnd = lambda *s: torch.randn(*s, generator=gen)                         # noqa: E731
    PQ = rnd(N, 2 * H1p)
    PQ[:, H1:H1p] = 50.0                                                     # pad columns: must stay out of the statistics
    PQ[:, H1p + H1:] = -70.0
    t = dict(PQ=PQ, W2=rnd(H2, H1) / H1 ** 0.5, b2=0.1 * rnd(H2), g1=1 + 0.2 * rnd(H1), be1=0.2 * rnd(H1), g2=1 + 0.2 * rnd(H2),
             be2=0.2 * rnd(H2), gout=rnd(N, H2))
    j, i = g.edge_index().cpu()
    # float64 restatement
    r = {n: v.double().requires_grad_(n != "gout") for n, v in t.items()}
    pre = r["PQ"][i, :H1] + r["PQ"][j, H1p:H1p + H1]
    a1 = F.gelu(F.layer_norm(pre, (H1,), r["g1"], r["be1"]))
    m = F.gelu(F.layer_norm(a1 @ r["W2"].t() + r["b2"], (H2,), r["g2"], r["be2"]))
    out = torch.zeros(N, H2, dtype=torch.float64).index_add(0, i, m)
    (out * r["gout"]).sum().backward()
    dPQ = r["PQ"].grad
    ref = dict(out=out.detach(), dP=dPQ[:, :H1], dQ=dPQ[:, H1p:H1p + H1], dW2=r["W2"].grad, db2=r["b2"].grad, dg1=r["g1"].grad,
               dbe1=r["be1"].grad, dg2=r["g2"].grad, dbe2=r["be2"].grad)
    assert int((out.abs().sum(1) == 0).sum()) == 1 and len(i) > 3 * 64 and int(torch.bincount(i).max()) == k + 1
    return g, {n: v.to(DEV) for n, v in t.items()}, ref, H1p


def run_fused(mode, g, t, H1, H1p, H2):
    from graphnet_amd import ops
    dt, cr = ops.mode_dtype(mode), ops.compact_rows(g)
    ln1, ln2 = (t["g1"], t["be1"]), (t["g2"], t["be2"])
    W2p, W2Tp = ops.pack_weight(t["W2"], [H1], dt, 32), ops.pack_weight(t["W2"].t(), [H2], dt, 32)
    out, st = ops.edgeconv_norm_fwd(mode, cr, t["PQ"], H1p, H1, H2, W2p, t["b2"], ln1, ln2)
    dPQ = torch.empty((g.N, 2 * H1p), dtype=dt, device=DEV)
    a1, dz2, dpre1, dg1, dbe1, dg2, dbe2 = ops.edgeconv_norm_bwd(mode, cr, t["PQ"], H1p, H1, H2, W2p, W2Tp, t["b2"], ln1, ln2, st,
                                                               t["gout"], dPQ[:, :H1p])
    dW2, db2 = ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
    ops.edgeconv_dq_gather(mode, cr.reverse_view(), dpre1, H1p, dPQ[:, H1p:])
    return dict(out=out, dP=dPQ[:, :H1], dQ=dPQ[:, H1p:H1p + H1], dW2=dW2[:, :H1], db2=db2, dg1=dg1, dbe1=dbe1, dg2=dg2, dbe2=dbe2)


def run_unfused(mode, g, t, H1, H1p, H2):
    """The chain of ``_DynEdgeGenericFunction`` without the switch (compact rows, bf16 edge rows in bf16 mode)."""
    from graphnet_amd import ops
    dt, ku, cr = ops.mode_dtype(mode), ops.gemm_kunit(mode), ops.compact_rows(g)
    lowp, r16 = ("only" if mode == 1 else "no"), mode == 1
    pre1 = ops.edge_gather_pre(t["PQ"], H1p, cr.ic, cr.jc, lowp=r16)
    a1, st1 = ops.rownorm_act_fwd(pre1, H1, "gelu", t["g1"], t["be1"], valid=cr.jc, cpad=H1p, lowp=lowp)
    z2 = ops.linear_fwd(mode, [(a1, H1p)], ops.pack_weight(t["W2"], [H1], dt, ku), H2, bias=t["b2"], out_cols=H2, out_lowp=r16)
    m, st2 = ops.rownorm_act_fwd(z2, H2, "gelu", t["g2"], t["be2"], valid=cr.jc, cpad=H2, lowp=lowp)
    out = cr.sum(m, H2)
    dz2, dg2, dbe2 = ops.rownorm_act_bwd(t["gout"], z2, H2, "gelu", t["g2"], t["be2"], st2, valid=cr.jc, gidx=cr.ic, cpad=H2, lowp=lowp)
    dW2, db2 = ops.linear_wgrad(mode, dz2, H2, [(a1, H1p)], with_bias=True)
    da1 = ops.linear_fwd(mode, [(dz2, H2)], ops.pack_weight(t["W2"].t(), [H2], dt, ku), H1, out_cols=H1p, out_lowp=r16)
    dpre1, dg1, dbe1 = ops.rownorm_act_bwd(da1, pre1, H1, "gelu", t["g1"], t["be1"], st1, valid=cr.jc, cpad=H1p, lowp=lowp)
    dPQ = torch.empty((g.N, 2 * H1p), dtype=dt, device=DEV)
    dPQ[:, :H1p] = cr.sum(dpre1, H1p)
    ops.edgeconv_dq_gather(mode, cr.reverse_view(), dpre1, H1p, dPQ[:, H1p:])
    return dict(out=out, dP=dPQ[:, :H1], dQ=dPQ[:, H1p:H1p + H1], dW2=dW2[:, :H1], db2=db2, dg1=dg1, dbe1=dbe1, dg2=dg2, dbe2=dbe2)


@pytest.mark.parametrize("k", [8, 9])
@pytest.mark.parametrize("H1,H2", [(128, 256), (336, 256), (40, 32)])
@pytest.mark.parametrize("name,mode", MODES)
def test_kernels_against_float64(name, mode, H1, H2, k):
    """out, dP, dQ, dW2, db2 and the four LayerNorm gradients; a centre without an edge gets exact zeros; two runs agree
    bit for bit."""
    from graphnet_amd import ops
    assert ops.edgeconv_norm_supported(mode, H1, H2) and not ops.edgeconv_norm_supported(mode, 400, 256)
    g, t, ref, H1p = kernel_case(mode, H1, H2, k)
    plan = ops.edgeconv_norm_plan(ops.compact_rows(g)).cpu()
    row_ptr = ops.compact_rows(g).row_ptr.cpu()
    rows = row_ptr[plan.long()][1:] - row_ptr[plan.long()][:-1]
    last = int(torch.nonzero(rows > 0).max())
    assert int((rows > 0).sum()) >= 3 and int(rows.max()) == (64 if k == 8 else 58) and 0 < int(rows[:last].min()) < 64
    fused, again, unfused = run_fused(mode, g, t, H1, H1p, H2), run_fused(mode, g, t, H1, H1p, H2), run_unfused(mode, g, t, H1, H1p, H2)
    assert torch.equal(fused["out"][0], torch.zeros_like(fused["out"][0]))                 # the single-pulse event
    for n in ref:
        assert torch.equal(fused[n], again[n]), n
        gate(f"{name} ({H1},{H2}) k={k} {n}", err(mode, fused[n], ref[n]), err(mode, unfused[n], ref[n]))


def model_reference(ref, x, gv, batch, graphs):
    h = torch.cat([x, gv[batch]], 1)
    skips = [h]
    for conv, (j, i) in zip(ref._conv_layers, graphs):
        msg = conv.nn(torch.cat([h[i], h[j] - h[i]], 1))
        h = torch.zeros(h.shape[0], msg.shape[1], dtype=h.dtype).index_add(0, i, msg)
        skips.append(h)
    return ref._post_processing(torch.cat(skips, 1))


@pytest.mark.parametrize("name,mode", MODES)
def test_dynedge_with_fused_norm_edge(name, mode):
    """The DynEdge DeepIce embeds (two of its layers), node-level output: forward and every parameter gradient with the
    switch on, teacher-forced on the graphs the device built, against the float64 restatement - and the same run with the
    switch off for the gate."""
    import graphnet_amd as g
    sizes = [4, 12, 30, 25, 40, 20]
    gen = torch.Generator().manual_seed(3)
    b = g.Batch(x=torch.randn(sum(sizes), 9, generator=gen).to(DEV))
    b.batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    b.n_pulses = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    b.ptr = torch.tensor([0] + sizes).cumsum(0).to(DEV)
    torch.manual_seed(4)
    m = g.DynEdge(9, nb_neighbours=9, dynedge_layer_sizes=[(128, 256), (336, 256)], post_processing_layer_sizes=[336, 192],
                  global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)
    ref = copy.deepcopy(m).double()
    m.to(DEV)
    w = torch.randn(sum(sizes), 192, generator=gen)
    errs = {}
    for fused in (False, True):
        m.set_backend(dtype=name, fused_norm_edge=fused)
        m.zero_grad(); ref.zero_grad()
        y, trace = m(b, return_trace=True)
        (y * w.to(DEV)).sum().backward()
        graphs = [tuple(t.edge_index().cpu()) for t in trace["graphs"]]
        yo = model_reference(ref, b.x.double().cpu(), trace["global_variables"].double().cpu(), b.batch.cpu(), graphs)
        (yo * w.double()).sum().backward()
        errs[fused] = {"y": err(mode, y, yo)}
        for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
            if po.grad is not None:
                errs[fused][kn] = err(mode, p.grad, po.grad)
    for n in errs[True]:
        gate(f"{name} model {n}", errs[True][n], errs[False][n])
