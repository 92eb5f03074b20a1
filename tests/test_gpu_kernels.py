"""GPU parity tests: every kernel of the C ABI against the CPU oracle (same seeded inputs).

Integer/index results must be bit-exact; fp32 mode within 1e-4 relative (of the tensor's max
magnitude); bf16 operand mode within 2e-2 (stated in each assert).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = [("fp32", 0, 1e-4), ("bf16", 1, 2e-2)]


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def norm_err(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _batch(n_events=12, seed=3):
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    return synthetic_icecube86_batch(n_events, seed=seed)


def _csr(b):
    ptr32 = b.ptr.to(torch.int32).to(DEV)
    batch32 = b.batch.to(torch.int32).to(DEV)
    return ptr32, batch32


def _oracle_table(oracle, x, ptr, k, cols, mode):
    nbr, _ = oracle.knn_table(x, k, ptr.long(), cols, mode)
    return nbr


def _cmp_table(table, nbr_oracle, k):
    got = table.nbr.cpu().numpy()
    exp = nbr_oracle.numpy()
    assert np.array_equal(got, exp[:, :k])
    if table.ovf is not None:
        assert np.array_equal(table.ovf.cpu().numpy(), exp[:, k])
        cnt = int(table.ovf_cnt.item())
        centres = np.nonzero(exp[:, k] >= 0)[0]
        assert cnt == len(centres)
        assert np.array_equal(table.ovf_centre.cpu().numpy()[:cnt], centres)
        assert np.array_equal(table.ovf_src.cpu().numpy()[:cnt], exp[centres, k])


# ------------------------------------------------------------------------------ k-NN
@pytest.mark.parametrize("mode", ["compat", "strict"])
@pytest.mark.parametrize("k", [8, 16, 3, 24])
def test_knn_bit_exact_synthetic(oracle, mode, k):
    from graphnet_amd import ops
    b = _batch(40, seed=11)
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(b.x.to(DEV), [0, 1, 2], batch32, ptr32, k, strict=(mode == "strict"))
    _cmp_table(t, _oracle_table(oracle, b.x, b.ptr, k, [0, 1, 2], mode), k)


def test_knn_reference_events_and_edge_index(oracle, golden):
    from graphnet_amd import ops
    ex, ev = golden["oracle_expected"], golden["reference_events"]
    for name in ("deepcore", "upgrade", "prometheus"):
        x = torch.from_numpy(ex[f"{name}_xstd"])
        ptr = torch.from_numpy(ev[f"{name}_ptr"])
        n = (ptr[1:] - ptr[:-1])
        batch32 = torch.repeat_interleave(torch.arange(len(n)), n).to(torch.int32).to(DEV)
        for mode in ("compat", "strict"):
            t = ops.knn_graph(x.to(DEV), [0, 1, 2], batch32, ptr.to(torch.int32).to(DEV), 8, strict=(mode == "strict"))
            exp = torch.from_numpy(ex[f"{name}_nbr_{mode}"])
            _cmp_table(t, exp, 8)
            ei = t.edge_index().cpu()
            assert torch.equal(ei, oracle.table_to_edge_index(exp))
            if mode == "compat":       # loader edge_index -> table round trip
                t2 = ops.table_from_edge_index(ei.to(DEV), x.shape[0], 8)
                _cmp_table(t2, exp, 8)


def test_loader_edge_index_any_order_any_degree_and_bad_indices(oracle):
    """PyG's EdgeConv (``components/layers.py:60``) takes edges in any order and with any in-degree; indices outside
    [0, N) are the caller's error.  The device pass validates both int64 rows before it writes anything."""
    from graphnet_amd import ops
    b = _batch(10, seed=21)
    N = int(b.x.shape[0])
    ei = oracle.knn_graph(b.x, 8, b.batch, [0, 1, 2])                       # grouped by target
    t_sorted = ops.table_from_edge_index(ei.to(DEV), N, 8)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(0))
    t_shuf = ops.table_from_edge_index(ei[:, perm].to(DEV), N, 8)           # any order: same neighbour SETS per target

    def rows(t):
        full = torch.cat([t.nbr.cpu(), t.ovf.cpu().unsqueeze(1)], dim=1)
        return torch.sort(full, dim=1).values
    assert torch.equal(rows(t_sorted), rows(t_shuf))
    # the shuffled table keeps, inside a target, the order the edges had in the input (stable grouping)
    order = torch.argsort(ei[1, perm], stable=True)
    again = ops.table_from_edge_index(ei[:, perm][:, order].to(DEV), N, 8)
    assert torch.equal(again.nbr, t_shuf.nbr) and torch.equal(again.ovf, t_shuf.ovf)
    # a loader graph with another k (here 12) than the backbone's nb_neighbours = 8: the table grows
    ei12 = oracle.knn_graph(b.x, 12, b.batch, [0, 1, 2])
    t12 = ops.table_from_edge_index(ei12.to(DEV), N, 8)
    assert t12.K >= 11 and torch.equal(t12.edge_index().cpu(), ei12)
    # out-of-range entries in either row, negative or too large, also beyond int32: ValueError, nothing written OOB
    for row, val in ((0, N), (1, N), (0, -1), (1, -5), (1, 2 ** 33 + 3), (0, 2 ** 40)):
        bad = ei.clone()
        bad[row, 17] = val
        with pytest.raises(ValueError):
            ops.table_from_edge_index(bad.to(DEV), N, 8)
    with pytest.raises(ValueError):
        ops.table_from_edge_index(torch.zeros((3, 4), dtype=torch.int64, device=DEV), N, 8)
    # and the device is still healthy: the valid input still converts
    assert torch.equal(ops.table_from_edge_index(ei.to(DEV), N, 8).nbr, t_sorted.nbr)


def test_knn_edge_cases(oracle):
    from graphnet_amd import ops
    # ragged: events of 1, 2, 3 nodes (degree n-1), > k duplicates, D = 4 columns, big event
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 30, 1500, 9, 2, 2300]            # > 1024 pulses: candidates split over 8 waves per tile
    x = rng.normal(size=(sum(sizes), 6)).astype(np.float32)
    x[40:60, :4] = x[39, :4]
    x[216:236, :4] = x[39, :4]                          # the same point again, in another wave's piece (ties)
    x[1600:1640, :4] = x[3000, :4]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    n = ptr[1:] - ptr[:-1]
    batch32 = torch.repeat_interleave(torch.arange(len(n)), n).to(torch.int32).to(DEV)
    xt = torch.from_numpy(x)
    for cols in ([0, 1, 2], [0, 1, 2, 3], [5, 1]):
        t = ops.knn_graph(xt.to(DEV), cols, batch32, ptr.to(torch.int32).to(DEV), 8)
        _cmp_table(t, _oracle_table(oracle, xt, ptr, 8, cols, "compat"), 8)
    for kk, mode in ((16, "strict"), (3, "compat")):
        t = ops.knn_graph(xt.to(DEV), [0, 1, 2], batch32, ptr.to(torch.int32).to(DEV), kk, strict=(mode == "strict"))
        _cmp_table(t, _oracle_table(oracle, xt, ptr, kk, [0, 1, 2], mode), kk)
    # strided view (latent features are a column slice of a wider row)
    wide = torch.zeros(x.shape[0], 64)
    wide[:, 10:16] = xt
    t = ops.knn_graph(wide.to(DEV)[:, 10:16], [0, 1, 2], batch32, ptr.to(torch.int32).to(DEV), 8)
    _cmp_table(t, _oracle_table(oracle, xt, ptr, 8, [0, 1, 2], "compat"), 8)


@pytest.mark.parametrize("case", ["normal", "dom_like", "collapsed", "outliers", "nan_inf"])
@pytest.mark.parametrize("k,strict,cols", [(16, False, [0, 1, 2]), (8, True, [0, 1, 2, 3]), (24, False, [4, 1])])
def test_knn_sorted_sweep_of_large_events_is_the_exhaustive_table(oracle, case, k, strict, cols):
    """Events of 1025..16384 pulses in batches that average >= 512 per event (BASELINE configs[4]): Morton sort + bounding-box
    pruning (knn_sort_kernel / knn_sweep_kernel) must return the exhaustive scan's table entry for entry - ties by index,
    duplicates, collapsed coordinates, outliers, NaN / inf coordinates; events outside the range stay on the old kernels."""
    from graphnet_amd import ops
    rng = np.random.default_rng(17 + k)
    sizes = [1025, 3000, 16384, 700, 16385, 2047, 5]
    N = sum(sizes)
    x = rng.normal(size=(N, 6)).astype(np.float32)
    if case == "dom_like":                              # ~30 pulses per position: the k-th distance is 0, ties decided by index
        pos = rng.normal(size=(300, 6)).astype(np.float32)
        x = pos[rng.integers(0, 300, size=N)]
    elif case == "collapsed":                           # every pulse of an event on a handful of points (trained coordinates)
        x = np.round(x * 0.6).astype(np.float32)
    elif case == "outliers":                            # the event's box is set by a few far points: all others share a cell
        x *= 1e-3
        x[rng.integers(0, N, size=40)] *= 1e6
    elif case == "nan_inf":
        x[rng.integers(0, N, size=60), rng.integers(0, 6, size=60)] = np.nan
        x[rng.integers(0, N, size=30), rng.integers(0, 6, size=30)] = np.inf
        x[rng.integers(0, N, size=30), rng.integers(0, 6, size=30)] = -np.inf
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    n = (ptr[1:] - ptr[:-1]).long()
    batch32 = torch.repeat_interleave(torch.arange(len(n)), n).to(torch.int32).to(DEV)
    xt = torch.from_numpy(x).to(DEV)
    a = ops.knn_graph(xt, cols, batch32, ptr.to(DEV), k, strict=strict, sweep=True)
    b = ops.knn_graph(xt, cols, batch32, ptr.to(DEV), k, strict=strict, sweep=False)
    assert torch.equal(a.nbr, b.nbr)
    if not strict:
        assert torch.equal(a.ovf, b.ovf)
    if case in ("normal", "dom_like") and k == 16:     # and the oracle itself on the smaller events (seconds on the CPU)
        sel = slice(0, sizes[0] + sizes[1])
        exp = _oracle_table(oracle, torch.from_numpy(x[sel]), ptr[:3].long(), k, cols, "strict" if strict else "compat").numpy()
        assert np.array_equal(a.nbr[sel].cpu().numpy(), exp[:, :k])
        assert np.array_equal(a.ovf[sel].cpu().numpy(), exp[:, k])


def test_reverse_adjacency(oracle):
    from graphnet_amd import ops
    b = _batch(10, seed=2)
    x = b.x.clone()
    x[5:20, :3] = x[4, :3]                      # force overflow rows
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(x.to(DEV), [0, 1, 2], batch32, ptr32, 8)
    t.build_reverse()
    N, K, S = t.N, 8, t.S
    nbr = t.nbr.cpu().numpy()
    cnt = int(t.ovf_cnt.item())
    assert cnt > 0
    osrc = t.ovf_src.cpu().numpy()[:cnt]
    rp, rr = t.rev_ptr.cpu().numpy(), t.rev_rows.cpu().numpy()
    exp = [[] for _ in range(N)]
    for i in range(N):
        for s in range(K):
            if nbr[i, s] >= 0:
                exp[nbr[i, s]].append(i * S + s)
    for q in range(cnt):
        exp[osrc[q]].append(N * S + q)
    assert rp[0] == 0 and rp[N] == sum(len(e) for e in exp)
    for j in range(N):
        assert sorted(rr[rp[j]:rp[j + 1]].tolist()) == sorted(exp[j])


@pytest.mark.parametrize("name,mode", [("fp32", 0), ("bf16", 1)])
def test_dq_gather_hub_nodes(oracle, name, mode):
    """Hub pulses (many pulses on one DOM -> the lowest-index ones are everybody's neighbours) have in-edge
    lists far longer than a wave: those lists are sorted at graph build (ascending row id) and the gather
    must still equal a plain index_add in ascending row order, twice bit-identically."""
    from graphnet_amd import ops
    b = _batch(30, seed=21)
    x = b.x.clone()
    ev = int((b.ptr[1:] - b.ptr[:-1]).argmax())
    lo, hi = int(b.ptr[ev]), int(b.ptr[ev + 1])
    assert hi - lo > 150
    x[lo:lo + 150, :3] = x[lo, :3]              # 150 pulses on one DOM
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(x.to(DEV), [0, 1, 2], batch32, ptr32, 8)
    t.build_reverse()
    rp, rr = t.rev_ptr.cpu().numpy(), t.rev_rows.cpu().numpy()
    deg = rp[1:] - rp[:-1]
    assert deg.max() > 100
    hub = int(deg.argmax())
    assert np.all(np.diff(rr[rp[hub]:rp[hub + 1]]) > 0), "hub list sorted ascending"
    dt = ops.act_dtype(mode)
    torch.manual_seed(9)
    H1p = 352
    dpre = torch.randn(t.rows, H1p).to(dt)
    dQ = torch.zeros(t.N, H1p, dtype=dt, device=DEV)
    ops.edgeconv_dq_gather(mode, t, dpre.to(DEV), H1p, dQ)
    dQ2 = torch.zeros_like(dQ)
    ops.edgeconv_dq_gather(mode, t, dpre.to(DEV), H1p, dQ2)
    assert torch.equal(dQ, dQ2)
    ref = torch.zeros(t.N, H1p, dtype=torch.float64)
    for j in range(t.N):
        rows = torch.from_numpy(rr[rp[j]:rp[j + 1]].astype(np.int64))
        if len(rows):
            ref[j] = dpre[rows].double().sum(0)
    assert rel_err(dQ, ref) < (1e-5 if mode == 0 else 1e-2)


def test_standardize_on_device_matches_oracle(oracle):
    """Detector._standardize as one HIP kernel against the ORACLE's restatement of the reference lambdas
    (oracle/detector_oracle.py; detector.py:64-77, icecube.py:21-48,84-170, prometheus.py:11-39): every non-log column
    bit-identical (they decide the k-NN graph), log10 columns to fp32 rounding of the device libm.  Also on the
    reference's own bundled events (the inputs of the golden k-NN tables)."""
    import graphnet_amd as g
    from oracle import detector_oracle as det_orc
    rng = np.random.default_rng(3)
    cases = (("IceCube86", g.IceCube86(), ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "rde", "pmt_area"]),
             ("IceCubeDeepCore", g.IceCubeDeepCore(), ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "rde", "pmt_area", "hlc"]),
             ("IceCubeUpgrade", g.IceCubeUpgrade(), ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "rde", "pmt_area", "string",
                                                     "pmt_number", "dom_number", "pmt_dir_x", "pmt_dir_y", "pmt_dir_z", "dom_type"]),
             ("Prometheus", g.Prometheus(), ["sensor_pos_x", "sensor_pos_y", "sensor_pos_z", "t"]))
    log_cols = {"IceCube86": {"charge"}, "IceCubeDeepCore": set(), "IceCubeUpgrade": {"charge"}, "Prometheus": set()}
    for name, det, names in cases:
        F = len(names)
        raw = torch.from_numpy(rng.uniform(-600, 600, size=(1000, F)).astype(np.float32))
        if "charge" in names:
            raw[:, names.index("charge")] = torch.from_numpy(rng.lognormal(0.3, 0.9, 1000).astype(np.float32))
        want = det_orc.standardize(name, raw, names)
        dev = det(raw.clone().to(DEV), names).cpu()
        for f, nm in enumerate(names):
            if nm in log_cols[name]:
                assert torch.allclose(dev[:, f], want[:, f], rtol=2e-6, atol=1e-7), (name, nm)
            else:
                assert torch.equal(dev[:, f], want[:, f]), (name, nm)
    with pytest.raises(KeyError):
        g.IceCube86()(raw.to(DEV), ["nope"] * F)


def test_standardize_reference_events_equal_golden_xstd(golden):
    """The reference's bundled events through gn_standardize == the *_xstd fixture (generated by the oracle's Detector
    restatement, tests/golden/make_fixtures.py), xyz columns bit for bit: the golden k-NN tables start from them."""
    import graphnet_amd as g
    ev, ex = golden["reference_events"], golden["oracle_expected"]
    ice = ["dom_x", "dom_y", "dom_z", "dom_time", "charge", "rde", "pmt_area"]
    upg = ice + ["string", "pmt_number", "dom_number", "pmt_dir_x", "pmt_dir_y", "pmt_dir_z", "dom_type"]
    for name, det, names in (("deepcore", g.IceCube86(), ice), ("upgrade", g.IceCubeUpgrade(), upg),
                             ("prometheus", g.Prometheus(), ["sensor_pos_x", "sensor_pos_y", "sensor_pos_z", "t"])):
        raw = torch.tensor(ev[f"{name}_x"], dtype=torch.float32)
        dev = det(raw.to(DEV), names).cpu()
        want = torch.from_numpy(ex[f"{name}_xstd"])
        assert torch.equal(dev[:, :3], want[:, :3]), name
        assert torch.allclose(dev, want, rtol=2e-6, atol=1e-7), name


# ------------------------------------------------------------------------------ globals
def test_graph_globals(oracle):
    from graphnet_amd import ops
    b = _batch(25, seed=4)
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(b.x.to(DEV), [0, 1, 2], batch32, ptr32, 8)
    gv = ops.graph_globals(b.x.to(DEV), ptr32, t, b.n_pulses.to(DEV)).cpu()
    ei = oracle.knn_graph(b.x, 8, b.batch, [0, 1, 2])
    m = oracle.DynEdgeOracle(7)
    exp = m.global_variables(b.x, ei, b.batch, b.n_pulses, len(b.n_pulses))
    assert torch.equal(gv[:, 7:11], exp[:, 7:11])             # homophily: integer counts -> exact
    assert (gv[:, 7:11] > 0).any()
    assert torch.allclose(gv, exp, rtol=1e-5, atol=1e-6)
    x0 = ops.concat_globals(b.x.to(DEV), gv.to(DEV), batch32, 32).cpu()
    assert torch.equal(x0[:, :7], b.x) and torch.equal(x0[:, 7:19], gv[b.batch]) and (x0[:, 19:] == 0).all()


def test_event_reductions_of_huge_events_do_not_depend_on_the_batch(oracle):
    """Pooling and the global variables reduce an event in slices of 1024 pulses folded in order.  A batch of a few huge
    events (BASELINE configs[4]) runs one workgroup per slice (scratch buffer), any other batch one workgroup per event
    that walks the slices: the SAME bits either way, and the same as the event gets inside a larger batch."""
    from graphnet_amd import ops
    from graphnet_amd.ops import _lib, _p, _st, _rows
    import ctypes
    sizes = [2500, 1, 1100, 0, 3000, 1024, 1025]
    gen = torch.Generator().manual_seed(12)
    N, C = sum(sizes), 256
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    y = torch.randn(N, C, generator=gen)
    y[5:900, 3] = y[4, 3]                                       # ties: the first occurrence must win in every path
    schemes = ["min", "max", "mean", "sum"]
    ref = torch.cat([oracle.GLOBAL_POOLINGS[s](y.double(), batch, len(sizes)) for s in schemes], 1)
    yd, ptrd = y.to(DEV), ptr.to(DEV)
    out_s, amin_s, amax_s = ops.segment_pool_fwd(yd, C, ptrd, schemes)          # sliced workgroups (B <= 64, N > 1024)
    B = len(sizes)
    out_p = torch.empty_like(out_s); amin_p = torch.empty_like(amin_s); amax_p = torch.empty_like(amax_s)
    c = ops._codes(schemes)
    _lib.check(_lib.lib().gn_segment_pool_fwd(_p(yd), _rows(yd, "x"), C, _p(ptrd), B, ctypes.cast(c, ctypes.c_void_p), 4,
                                              _p(out_p), _p(amin_p), _p(amax_p), _st()))          # one workgroup per event
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_p) and torch.equal(amin_s, amin_p) and torch.equal(amax_s, amax_p)
    assert torch.allclose(out_s.cpu().double(), ref, rtol=2e-5, atol=1e-4)
    assert int(amin_s[0, 3]) == 4 or float(y[int(amin_s[0, 3]), 3]) < float(y[4, 3])
    # the same events inside a batch of 80 (> 64 events: never sliced workgroups)
    more = [3] * 73
    ptr2 = torch.tensor(np.concatenate([[0], np.cumsum(sizes + more)]), dtype=torch.int32)
    y2 = torch.cat([y, torch.randn(sum(more), C, generator=gen)])
    out2, amin2, amax2 = ops.segment_pool_fwd(y2.to(DEV), C, ptr2.to(DEV), schemes)
    assert torch.equal(out2[:B], out_s) and torch.equal(amin2[:B], amin_s)
    # global variables: 3 events of 1500 / 40 / 2600 pulses, sliced workgroups against the plain entry and the oracle
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    b = synthetic_icecube86_batch(3, seed=9, count_range=(40, 2600))
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(b.x.to(DEV), [0, 1, 2], batch32, ptr32, 8)
    gv = ops.graph_globals(b.x.to(DEV), ptr32, t, b.n_pulses.to(DEV))
    gv_p = torch.empty_like(gv)
    xd = b.x.to(DEV)
    _lib.check(_lib.lib().gn_graph_globals(_p(xd), _rows(xd, "x"), 7, _p(ptr32), 3, _p(t.nbr), _p(t.ovf), t.K,
                                           _p(b.n_pulses.to(DEV)), _p(gv_p), _st()))
    torch.cuda.synchronize()
    assert torch.equal(gv, gv_p)
    ei = oracle.knn_graph(b.x, 8, b.batch, [0, 1, 2])
    exp = oracle.DynEdgeOracle(7).global_variables(b.x, ei, b.batch, b.n_pulses, 3)
    assert torch.equal(gv.cpu()[:, 7:11], exp[:, 7:11]) and torch.allclose(gv.cpu(), exp, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------ dense layers
@pytest.mark.parametrize("name,mode,tol", MODES)
def test_linear_fwd_segments_and_epilogues(name, mode, tol):
    from graphnet_amd import ops
    torch.manual_seed(0)
    M = 1000
    widths = [19, 256, 64]
    xs = [torch.randn(M, ops.round_up(w, 32)) for w in widths]
    for x, w in zip(xs, widths):
        x[:, w:] = 0
    W = torch.randn(336, sum(widths)) * 0.1
    bias = torch.randn(336)
    ref = torch.cat([x[:, :w] for x, w in zip(xs, widths)], 1) @ W.t() + bias
    segs = [(x.to(DEV), w if w % 4 == 0 else ops.round_up(w, 32)) for x, w in zip(xs, widths)]
    # the 19-wide segment is passed zero-padded to 32 columns: pack W accordingly
    Wfull = torch.zeros(336, sum(s[1] for s in segs))
    off = offp = 0
    for (x, wp), w in zip(segs, widths):
        Wfull[:, offp:offp + w] = W[:, off:off + w]
        off += w; offp += wp
    Wp = ops.pack_weight(Wfull.to(DEV), [s[1] for s in segs], ops.mode_dtype(mode), ops.gemm_kunit(mode))
    y = ops.linear_fwd(mode, segs, Wp, 336, bias=bias.to(DEV))
    assert rel_err(y, ref) < tol, f"{name}: plain"
    y = ops.linear_fwd(mode, segs, Wp, 336, bias=bias.to(DEV), relu=True)
    assert rel_err(y, ref.relu()) < tol, f"{name}: relu"
    gate = torch.randn(M, 336)
    y = ops.linear_fwd(mode, segs, Wp, 336, bias=bias.to(DEV), gate=gate.to(DEV))
    assert rel_err(y, ref * (gate > 0)) < tol, f"{name}: gate"
    base = torch.randn(M, 400)
    out = base.clone().to(DEV)
    ops.linear_fwd(mode, segs, Wp, 336, bias=bias.to(DEV), out=out[:, 32:368], accum=True)
    exp = base.clone(); exp[:, 32:368] += ref
    assert rel_err(out, exp) < tol, f"{name}: accumulate into a strided view"
    if mode == 1:
        y = ops.linear_fwd(mode, segs, Wp, 336, bias=bias.to(DEV), out_lowp=True)
        assert y.dtype == torch.bfloat16 and rel_err(y.float(), ref) < tol
        # bf16 activation rows (what the model passes in bf16 mode): 16-byte granularity = 8 columns;
        # the result must equal the fp32-row call on the same (bf16-representable) values bit for bit
        xs16 = [x.bfloat16() for x in xs]
        segs16 = [(x.to(DEV), s[1]) for x, s in zip(xs16, segs)]
        segs32 = [(x.float().to(DEV), s[1]) for x, s in zip(xs16, segs)]
        gate16 = gate.bfloat16().to(DEV)
        ya = ops.linear_fwd(mode, segs16, Wp, 336, bias=bias.to(DEV), gate=gate16)
        yb = ops.linear_fwd(mode, segs32, Wp, 336, bias=bias.to(DEV), gate=gate16.float())
        assert torch.equal(ya, yb), "bf16 rows / bf16 gate must not change the arithmetic"
        out16 = base.bfloat16().to(DEV)
        ops.linear_fwd(mode, segs16, Wp, 336, bias=bias.to(DEV), out=out16[:, 32:368], accum=True)
        assert out16.dtype == torch.bfloat16 and rel_err(out16.float(), exp) < tol, "accumulate into a bf16 view"
        assert torch.equal(out16[:, :32].float().cpu(), base.bfloat16()[:, :32].float()), "outside the view untouched"


@pytest.mark.parametrize("name,mode,tol", MODES)
def test_linear_wgrad_and_colsum(name, mode, tol):
    from graphnet_amd import ops
    torch.manual_seed(1)
    M = 5000
    dY = torch.randn(M, 336)
    xa, xb = torch.randn(M, 32), torch.randn(M, 256)
    xa[:, 19:] = 0
    ref = dY.t() @ torch.cat([xa, xb], 1)
    dW, db = ops.linear_wgrad(mode, dY.to(DEV), 336, [(xa.to(DEV), 32), (xb.to(DEV), 256)], with_bias=True)
    assert rel_err(dW, ref) < tol
    assert rel_err(db, dY.sum(0)) < (1e-5 if mode == 0 else 1e-2)       # bf16 mode: dY rounded to bf16 in the ones-MFMA
    dW2 = ops.linear_wgrad(mode, dY.to(DEV), 336, [(xa.to(DEV), 32), (xb.to(DEV), 256)])
    assert torch.equal(dW, dW2), "split reduction must be bitwise reproducible"
    # wide / ragged shapes: N1 not a multiple of the tile, several k tiles, M not a multiple of 64
    dY3, x3 = torch.randn(1237, 708), torch.randn(1237, 260)
    dW3, db3 = ops.linear_wgrad(mode, dY3.to(DEV), 708, [(x3.to(DEV), 260)], with_bias=True)
    assert rel_err(dW3, dY3.t() @ x3) < tol and rel_err(db3, dY3.sum(0)) < (1e-5 if mode == 0 else 1e-2)
    cs = ops.colsum(dY.to(DEV), 336)
    assert rel_err(cs, dY.sum(0)) < 1e-5
    if mode == 1:
        # bf16 dY / X rows: identical arithmetic to fp32 rows holding the same bf16-representable values
        dY16, xa16, xb16 = dY.bfloat16(), xa.bfloat16(), xb.bfloat16()
        a = ops.linear_wgrad(mode, dY16.to(DEV), 336, [(xa16.to(DEV), 32), (xb16.to(DEV), 256)], with_bias=True)
        b_ = ops.linear_wgrad(mode, dY16.float().to(DEV), 336, [(xa16.float().to(DEV), 32), (xb16.float().to(DEV), 256)],
                              with_bias=True)
        assert torch.equal(a[0], b_[0])
        # bias gradient: bf16 dY rides along as a ones block of the MFMA, fp32 dY takes the colsum pass (the ones block
        # would cost 16 registers the fp32 staging needs) - same values, another summation order
        assert rel_err(a[1], b_[1]) < 1e-5
        c = ops.linear_wgrad(mode, dY16.to(DEV), 336, [(xa16.float().to(DEV), 32), (xb16.float().to(DEV), 256)])
        assert torch.equal(c, a[0]), "mixed bf16 dY / fp32 X rows"


def test_weights_stationary_gemm_matches_tiled():
    """A/B: gemm_v2.hip (persistent, W in registers) against the tiled kernel (GN_DISABLE_V2=1) on the
    shapes the model uses: same MFMA sequence per output -> fp32 outputs equal, bf16 outputs equal."""
    import os
    from graphnet_amd import ops
    mode, dt = 1, torch.bfloat16
    torch.manual_seed(4)
    M = 5003                                           # ragged last tile
    cases = [  # (K real, K pitch, N, bias, relu, gate, out bf16)
        (256, 256, 704, True, False, False, True),     # P|Q projection
        (24, 32, 256, True, False, False, True),       # layer-1 projection (17 features + pad)
        (336, 336, 256, True, True, False, False),     # post-MLP layer 2 -> fp32 (pooling input)
        (256, 256, 336, False, False, True, True),     # d(post layer 1 output), relu gate
        (336, 336, 1024, False, False, False, True),   # d(skip-cat input)
        (256, 256, 100, True, True, False, False),     # ragged N, fp32
    ]
    for (K, ldk, N, has_b, relu, has_g, lowp) in cases:
        a = torch.randn(M, ldk).bfloat16()
        a[:, K:] = 0
        W = torch.randn(N, K) * 0.1
        bias = torch.randn(N).to(DEV) if has_b else None
        gate = torch.randn(M, ops.round_up(N, 8)).bfloat16().to(DEV) if has_g else None
        Wp = ops.pack_weight(W.to(DEV), [K], dt, ops.gemm_kunit(mode))
        res = {}
        for tag, flag in (("v2", "0"), ("v1", "1")):
            os.environ["GN_DISABLE_V2"] = flag
            res[tag] = ops.linear_fwd(mode, [(a.to(DEV), K)], Wp, N, bias=bias, relu=relu, gate=gate, out_lowp=lowp,
                                      out_cols=ops.round_up(N, 8))
            torch.cuda.synchronize()
        os.environ["GN_DISABLE_V2"] = "0"
        ref = a[:, :K].float() @ W.bfloat16().float().t()
        if has_b:
            ref = ref + bias.cpu()
        if relu:
            ref = ref.relu()
        if has_g:
            ref = ref * (gate.cpu()[:, :N].float() > 0)
        assert rel_err(res["v1"][:, :N], ref) < 2e-2, (K, N, "tiled vs torch")
        assert torch.equal(res["v2"][:, :N], res["v1"][:, :N]), (K, N, "stationary vs tiled")
        assert res["v2"].dtype == (dt if lowp else torch.float32)
    # accumulate into a bf16 view (input-gradient GEMMs): C = RNE(C_old + A.W^T), one rounding in both kernels
    a = torch.randn(M, 352).bfloat16().to(DEV)
    Wp = ops.pack_weight((torch.randn(256, 352) * 0.1).to(DEV), [352], dt, ops.gemm_kunit(mode))
    base = torch.randn(M, 1056).bfloat16()
    res = {}
    for tag, flag in (("v2", "0"), ("v1", "1")):
        os.environ["GN_DISABLE_V2"] = flag
        c = base.clone().to(DEV)
        ops.linear_fwd(mode, [(a, 352)], Wp, 256, out=c[:, 288:544], accum=True)
        torch.cuda.synchronize()
        res[tag] = c
    os.environ["GN_DISABLE_V2"] = "0"
    assert torch.equal(res["v2"], res["v1"])
    assert torch.equal(res["v2"][:, :288].cpu(), base[:, :288]) and torch.equal(res["v2"][:, 544:].cpu(), base[:, 544:])
    assert not torch.equal(res["v2"][:, 288:544].cpu(), base[:, 288:544])


# ------------------------------------------------------------------------------ EdgeConv
def _edgeconv_case(oracle, k=8, F=32, H1=336, H2=256, n_events=14, seed=6, dup=True):
    b = _batch(n_events, seed=seed)
    x3 = b.x.clone()
    if dup:
        x3[3:3 + k + 6, :3] = x3[2, :3]        # > k duplicates -> overflow rows
    torch.manual_seed(seed)
    N = x3.shape[0]
    x = torch.randn(N, F)
    mlp = torch.nn.Sequential(torch.nn.Linear(2 * F, H1), torch.nn.ReLU(), torch.nn.Linear(H1, H2), torch.nn.ReLU())
    ei = oracle.knn_graph(x3, k, b.batch, [0, 1, 2])
    return b, x3, x, mlp, ei


@pytest.mark.parametrize("name,mode,tol", MODES)
@pytest.mark.parametrize("k,F,H1,H2", [(8, 32, 336, 256), (8, 256, 336, 256), (16, 64, 128, 256), (5, 32, 100, 96), (8, 32, 344, 256)])
def test_edgeconv_forward(oracle, name, mode, tol, k, F, H1, H2):
    from graphnet_amd import ops
    b, x3, x, mlp, ei = _edgeconv_case(oracle, k=k, F=F, H1=H1, H2=H2)
    ref = oracle.edge_conv(x, ei, mlp, "add").detach()
    ptr32, batch32 = _csr(b)
    t = ops.knn_graph(x3.to(DEV), [0, 1, 2], batch32, ptr32, k)
    assert int(t.ovf_cnt.item()) > 0
    dt = ops.mode_dtype(mode)
    W1, b1, W2, b2 = [p.detach().to(DEV) for p in (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)]
    H1p = ops.round_up(H1, 32)
    Wpq = torch.zeros(2 * H1p, F, device=DEV)
    Wpq[:H1] = W1[:, :F] - W1[:, F:]
    Wpq[H1p:H1p + H1] = W1[:, F:]
    bpq = torch.zeros(2 * H1p, device=DEV); bpq[:H1] = b1
    PQ = ops.linear_fwd(mode, [(x.to(DEV), F)], ops.pack_weight(Wpq, [F], dt, ops.gemm_kunit(mode)), 2 * H1p, bias=bpq, out_lowp=(mode == 1))
    out, _mask, coords = ops.edgeconv_fwd(mode, t, PQ, H1p, ops.pack_weight(W2, [H1], dt), b2, H2,
                                          coord_cols=[0, 1, 2, 5], H1=H1)
    assert out.dtype == ops.act_dtype(mode)
    assert rel_err(out, ref) < tol, name
    # fp32 copy of the k-NN coordinate columns: the unrounded values of the same result
    assert coords.dtype == torch.float32 and rel_err(coords[:, :4], ref[:, [0, 1, 2, 5]]) < tol
    if mode == 0:
        assert torch.equal(coords[:, :4], out[:, [0, 1, 2, 5]])
    else:
        # bf16 out = RNE of the fp32 value; centres with an overflow (k+1-th) neighbour add that row to the
        # already rounded sum (second rounding), so they are only equal to one bf16 ulp
        plain = (t.ovf < 0)
        assert torch.equal(coords[plain][:, :4].bfloat16(), out[plain][:, [0, 1, 2, 5]])
        assert rel_err(coords[:, :4], out[:, [0, 1, 2, 5]].float()) < 1e-2


@pytest.mark.parametrize("name,mode,tol", MODES)
def test_single_layer_model_forward_backward(oracle, name, mode, tol):
    """One DynEdgeConv + post MLP + 4-way pooling + readout, fwd and all gradients."""
    import graphnet_amd as g
    b = _batch(9, seed=8)
    b.x[3:16, :3] = b.x[2, :3]
    kw = dict(dynedge_layer_sizes=[(128, 256)], global_pooling_schemes=["min", "max", "mean", "sum"])
    torch.manual_seed(3)
    ref = oracle.DynEdgeOracle(7, **kw)
    ei = oracle.knn_graph(b.x, 8, b.batch, [0, 1, 2])
    yo = ref(b.x, ei, b.batch, b.n_pulses)
    w = torch.randn_like(yo)
    (yo * w).sum().backward()
    m = g.DynEdge(7, **kw)
    m.load_state_dict(ref.state_dict())
    m.to(DEV).set_backend(dtype=name)
    y = m(b.to(DEV))
    (y * w.to(DEV)).sum().backward()
    assert rel_err(y, yo.detach()) < tol
    # fp32: max-abs relative 1e-3; bf16: relu gates downstream of rounded activations may flip for
    # single elements, so the bf16 gate is on the Frobenius-norm relative error (5e-2)
    for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, kn
        if mode == 0:
            assert rel_err(p.grad, po.grad) < 1e-3, f"{name}: grad {kn}"
        else:
            assert norm_err(p.grad, po.grad) < 5e-2, f"{name}: grad {kn}"


@pytest.mark.parametrize("act,norm", [("gelu", False), (None, True), ("gelu", True)])
@pytest.mark.parametrize("name,mode,tol", MODES)
def test_gelu_layernorm_variants(oracle, name, mode, tol, act, norm):
    """DynEdge(activation_layer="gelu", add_norm_layer=True) (dynedge.py:160-167,198-231) on the unfused
    kernels of csrc/generic.hip: two DynEdgeConv layers (teacher-forced on the graphs the device built),
    post MLP, pooling, read-out; output and every gradient (incl. LayerNorm weight / bias) vs the oracle."""
    import graphnet_amd as g
    b = _batch(7, seed=31)
    b.x[3:16, :3] = b.x[2, :3]
    kw = dict(dynedge_layer_sizes=[(64, 128), (96, 128)], post_processing_layer_sizes=[96, 64], readout_layer_sizes=[32],
              global_pooling_schemes=["min", "max", "mean", "sum"], activation_layer=act, add_norm_layer=norm)
    torch.manual_seed(5)
    ref = oracle.DynEdgeOracle(7, **kw)
    m = g.DynEdge(7, **kw)
    m.load_state_dict(ref.state_dict())
    m.to(DEV).set_backend(dtype=name)
    y, trace = m(b.to(DEV), return_trace=True)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    bc = b.to("cpu")
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], oracle.knn_graph(bc.x, 8, bc.batch, [0, 1, 2]))
    yo = ref(bc.x, forced[0], bc.batch, bc.n_pulses, forced_edges=forced)
    (yo * w).sum().backward()
    assert rel_err(y, yo.detach()) < tol
    for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, kn
        if mode == 0:
            assert rel_err(p.grad, po.grad) < 2e-3, f"{name}: grad {kn}"
        else:
            assert norm_err(p.grad, po.grad) < 5e-2, f"{name}: grad {kn}"


@pytest.mark.parametrize("name,mode,tol", MODES)
def test_dynedge_jinst_backbone(oracle, name, mode, tol):
    """DynEdgeJINST (models/gnn/dynedge_jinst.py:16-161): LeakyReLU edge MLPs, nn2 without activation, pooling
    order max/min/sum/mean, homophily + pulse count appended; same state-dict keys as the reference class."""
    import graphnet_amd as g
    b = _batch(6, seed=41)
    torch.manual_seed(8)
    ref = oracle.DynEdgeJINSTOracle(7, layer_size_scale=2)
    m = g.DynEdgeJINST(7, layer_size_scale=2)
    assert sorted(m.state_dict().keys()) == sorted(ref.state_dict().keys())
    m.load_state_dict(ref.state_dict())
    m.to(DEV).set_backend(dtype=name)
    y, trace = m(b.to(DEV), return_trace=True)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(2))
    (y * w.to(DEV)).sum().backward()
    bc = b.to("cpu")
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], oracle.knn_graph(bc.x, 8, bc.batch, [0, 1, 2]))
    yo = ref(bc.x, forced[0], bc.batch, bc.n_pulses, forced_edges=forced)
    (yo * w).sum().backward()
    assert y.shape == yo.shape == (6, ref.nb_outputs)
    assert rel_err(y, yo.detach()) < tol
    for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, kn
        err = rel_err(p.grad, po.grad) if mode == 0 else norm_err(p.grad, po.grad)
        # bf16: Frobenius-norm gate; 1e-1 because leaky relu passes every (rounded) activation on through four
        # layers - the first layer's small [64, 14] weight sees the accumulated bf16 noise (measured 7e-2)
        assert err < (2e-3 if mode == 0 else 1e-1), f"{name}: grad {kn}: {err}"


@pytest.mark.parametrize("aggr", ["add", "mean", "max", "add_leaky", "add_unfused"])
@pytest.mark.parametrize("name,mode,tol", MODES)
def test_standalone_dynedgeconv_aggregations(oracle, name, mode, tol, aggr):
    """graphnet_amd.DynEdgeConv (components/layers.py:20-69; reference default aggr="max") against the oracle's
    EdgeConv: output, gradient w.r.t. x and the MLP, and the re-clustered graph of the new features.  "add" with ReLU
    or LeakyReLU (add_leaky) runs on the fused edge kernels, add_unfused on the edge-row kernels (set_backend(fused=False))."""
    import graphnet_amd as g
    from graphnet_amd import ops
    b, x3, x, _mlp, ei = _edgeconv_case(oracle, k=8, F=24, H1=96, H2=64, n_events=8, seed=17)
    torch.manual_seed(4)
    variant, aggr = aggr, aggr.split("_")[0]
    act = torch.nn.LeakyReLU() if variant in ("max", "add_leaky") else torch.nn.ReLU()
    mlp = torch.nn.Sequential(torch.nn.Linear(48, 96), act, torch.nn.Linear(96, 64), act)
    xo = x.clone().requires_grad_()
    ref = oracle.edge_conv(xo, ei, mlp, aggr)
    w = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3))
    (ref * w).sum().backward()
    import copy
    conv = g.DynEdgeConv(copy.deepcopy(mlp), aggr=aggr, nb_neighbors=8, features_subset=slice(0, 3)).to(DEV).set_backend(name)
    conv.set_backend(fused=variant != "add_unfused")
    conv.zero_grad()
    xd = x.clone().to(DEV).requires_grad_()
    ops.enable_timers(True)
    out, table = conv(xd, ei.to(DEV), b.batch.to(DEV))
    (out * w.to(DEV)).sum().backward()
    used = ops.timer_summary(detail=True)
    ops.enable_timers(False)
    fused_ran = any(k.startswith(("edgeconv_fwd[", "edgeconv_leaky_fwd[")) for k in used)
    assert fused_ran == (variant in ("add", "add_leaky")), (variant, list(used))
    assert rel_err(out, ref.detach()) < tol, aggr
    gerr = (lambda a, c: rel_err(a, c)) if mode == 0 else (lambda a, c: norm_err(a, c))
    # bf16 + max: near-equal messages can swap their arg under bf16 GEMM noise, which re-routes whole gradient rows
    gt = 2e-3 if mode == 0 else (1e-1 if aggr == "max" else 5e-2)
    assert gerr(xd.grad, xo.grad) < gt, (aggr, "dx")
    for (kn, p), (_, po) in zip(conv.nn.named_parameters(), mlp.named_parameters()):
        assert gerr(p.grad, po.grad) < gt, (aggr, kn)
    # the returned graph = k-NN of the NEW features' first three columns (layers.py:63-67), bit-exact
    exp = oracle.knn_graph(out.detach().float().cpu(), 8, b.batch, slice(0, 3))
    assert torch.equal(table.edge_index().cpu(), exp)
    with pytest.raises(NotImplementedError):
        g.DynEdgeConv(torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Tanh(), torch.nn.Linear(4, 4), torch.nn.Tanh()))


# ------------------------------------------------------------------------------ pooling
def test_segment_pool_forward_backward(oracle):
    from graphnet_amd import ops
    torch.manual_seed(2)
    sizes = [5, 1, 40, 0, 17]
    N = sum(sizes)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = torch.randn(N, 256).relu().requires_grad_()
    schemes = ["min", "max", "mean", "sum"]
    ref = torch.cat([oracle.GLOBAL_POOLINGS[s](x, batch, len(sizes)) for s in schemes], 1)
    out, amin, amax = ops.segment_pool_fwd(x.detach().to(DEV), 256, ptr.to(DEV), schemes)
    assert torch.allclose(out.cpu(), ref.detach(), rtol=1e-5, atol=1e-6)
    assert (out.cpu()[3] == 0).all()                            # empty segment -> 0
    # backward on strictly positive rows (unique arg): compare with autograd through the oracle
    x2 = (torch.rand(N, 256) + 0.1).requires_grad_()
    ref2 = torch.cat([oracle.GLOBAL_POOLINGS[s](x2, batch, len(sizes)) for s in schemes], 1)
    gw = torch.randn_like(ref2)
    (ref2 * gw).sum().backward()
    out2, amin, amax = ops.segment_pool_fwd(x2.detach().to(DEV), 256, ptr.to(DEV), schemes)
    dx = ops.segment_pool_bwd(gw.to(DEV), 256, ptr.to(DEV), batch.to(torch.int32).to(DEV), N, schemes, amin, amax,
                              x2.detach().to(DEV))
    assert torch.allclose(dx.cpu(), x2.grad, rtol=1e-5, atol=1e-6)


def test_persistent_kernels_match_generic_kernels(oracle):
    """A/B: the persistent operand-stationary bf16 kernels (edgeconv_v2.hip) against the generic
    tiled kernels (GN_DISABLE_V2=1) on identical bf16 inputs: fp32 results (weight gradients) agree
    to 1e-4 of the tensor's max (accumulation order), bf16 tensors (out, dP|dQ, dpre) to one bf16 ulp."""
    import os
    from graphnet_amd import ops
    mode, dt = 1, torch.bfloat16
    # k <= 8 -> 8 slots per centre (uint8 slot masks), 9 <= k <= 16 -> 16 slots (uint16 masks)
    # H1 = 336: the contraction stops after 21 of the 22 k-steps of the padded layout; 340: real columns in the last one
    for (kk, F, H1, H2, n_events) in ((8, 256, 336, 256, 60), (8, 32, 128, 256, 20), (16, 256, 336, 256, 40),
                                      (11, 32, 128, 256, 20), (8, 64, 340, 256, 30), (16, 64, 348, 256, 20)):
        b, x3, x, mlp, ei = _edgeconv_case(oracle, k=kk, F=F, H1=H1, H2=H2, n_events=n_events, seed=12)
        ptr32, batch32 = _csr(b)
        g = ops.knn_graph(x3.to(DEV), [0, 1, 2], batch32, ptr32, kk)
        assert int(g.ovf_cnt.item()) > 0
        N, H1p = g.N, ops.round_up(H1, 32)
        W1, b1, W2, b2 = [p.detach().to(DEV) for p in (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)]
        Wpq = torch.zeros(2 * H1p, F, device=DEV)
        Wpq[:H1] = W1[:, :F] - W1[:, F:]
        Wpq[H1p:H1p + H1] = W1[:, F:]
        bpq = torch.zeros(2 * H1p, device=DEV); bpq[:H1] = b1
        PQ = ops.linear_fwd(mode, [(x.to(DEV), F)], ops.pack_weight(Wpq, [F], dt, ops.gemm_kunit(mode)), 2 * H1p, bias=bpq, out_lowp=True)
        W2p, W2Tp = ops.pack_weight(W2, [H1], dt), ops.pack_weight(W2.t().contiguous(), [H2], dt)
        torch.manual_seed(5)
        gout = torch.randn(N, H2, device=DEV).to(dt)            # activations / gradients are bf16 in bf16 mode
        res = {}
        for tag, flag in (("v2", "0"), ("v1", "1")):
            os.environ["GN_DISABLE_V2"] = flag
            out, saved = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2, H2, H1=H1)
            dW2, db2 = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, gout, saved)
            dPQ = torch.zeros(N, 2 * H1p, dtype=dt, device=DEV)
            dpre = torch.zeros(g.rows, H1p, dtype=dt, device=DEV)
            ops.edgeconv_bwd(mode, g, PQ, H1p, H2, gout, saved, W2Tp, dpre, dPQ[:, :H1p])
            ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
            torch.cuda.synchronize()
            res[tag] = dict(out=out, dW2=dW2, db2=db2, dPQ=dPQ, dpre=dpre.float())
        os.environ["GN_DISABLE_V2"] = "0"
        # The two kernel families accumulate in different orders, so a pre-activation within rounding of 0
        # can get a different relu bit (a handful of elements per million); gates: Frobenius-norm error, and
        # the fraction of elements that differ by more than 1 % of the tensor's max.
        def close(a, c, what):
            d = (a.float() - c.float()).abs()
            frac = float((d > 1e-2 * c.float().abs().max()).float().mean())
            tol = 5e-3 if a.dtype == torch.bfloat16 or what == "dpre" else 2e-3     # bf16: one-ulp noise
            assert norm_err(a, c) < tol and frac < 1e-4, (kk, F, H1, what, norm_err(a, c), frac)
        for k in ("dW2", "db2", "out", "dPQ"):
            close(res["v2"][k], res["v1"][k], k)
        nrows = N * g.S + int(g.ovf_cnt.item())
        close(res["v2"]["dpre"][:nrows], res["v1"]["dpre"][:nrows], "dpre")


@pytest.mark.parametrize("sizes", [[1], [3], [2, 9], [65], [7, 1, 130]])
@pytest.mark.parametrize("kk,H1", [(8, 336), (8, 128), (12, 352)])
def test_persistent_kernels_on_tiny_batches(sizes, kk, H1):
    """The persistent bf16 edge kernels on batches smaller than one tile range: single pulses, events with fewer pulses
    than k (empty slots), a pulse count that is not a multiple of the 8 (4) centres of a tile.  Their loops look two
    or three tiles ahead without branches (clamped loads, slack rows in the saved buffer): every result must still
    equal the generic kernels' on the same inputs, and nothing may be read or written out of bounds."""
    import os
    from graphnet_amd import ops
    mode, dt, F, H2 = 1, torch.bfloat16, 32, 256
    gen = torch.Generator().manual_seed(100 + sum(sizes) + kk)
    N = sum(sizes)
    x3 = torch.randn(N, 3, generator=gen)
    ptr = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32)
    batch = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes))
    g = ops.knn_graph(x3.to(DEV), [0, 1, 2], batch.to(DEV), ptr.to(DEV), kk)
    H1p = ops.round_up(H1, 32)
    PQ = (torch.randn(N, 2 * H1p, generator=gen) * 0.5).to(DEV).to(dt)
    PQ[:, H1:H1p] = 0
    PQ[:, H1p + H1:] = 0
    W2 = (torch.randn(H2, H1, generator=gen) * 0.1).to(DEV)
    b2 = (torch.randn(H2, generator=gen) * 0.1).to(DEV)
    W2p, W2Tp = ops.pack_weight(W2, [H1], dt), ops.pack_weight(W2.t().contiguous(), [H2], dt)
    gout = torch.randn(N, H2, generator=gen).to(DEV).to(dt)
    res = {}
    for tag, flag in (("v2", "0"), ("v1", "1")):
        os.environ["GN_DISABLE_V2"] = flag
        try:
            out, saved = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2, H2, H1=H1)
            dW2, db2 = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, gout, saved)
            dPQ = torch.zeros(N, 2 * H1p, dtype=dt, device=DEV)
            dpre = torch.zeros(max(g.rows, 1), H1p, dtype=dt, device=DEV)
            ops.edgeconv_bwd(mode, g, PQ, H1p, H2, gout, saved, W2Tp, dpre, dPQ[:, :H1p])
            ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
            torch.cuda.synchronize()
        finally:
            os.environ["GN_DISABLE_V2"] = "0"
        res[tag] = dict(out=out.float(), dW2=dW2, db2=db2, dPQ=dPQ.float())
    for k in ("out", "dW2", "db2", "dPQ"):
        a, c = res["v2"][k], res["v1"][k]
        assert torch.isfinite(a).all()
        scale = float(c.abs().max()) + 1e-6
        assert float((a - c).abs().max()) <= 2e-2 * scale, (sizes, kk, H1, k, float((a - c).abs().max()), scale)


@pytest.mark.parametrize("name,mode,tol", MODES)
def test_dynedge_as_embedded_in_deepice(oracle, name, mode, tol):
    """The DynEdge that ``DeepIce(include_dynedge=True)`` embeds (``models/gnn/icemix.py:100-118``): 9 neighbours in
    the re-clustering, GELU, LayerNorm, no pooling, no read-out (node-level features), fed with the loader's
    6-neighbour graph over (x, y, z, t)."""
    import graphnet_amd as g
    b = _batch(6, seed=23)
    kw = dict(nb_neighbours=9, post_processing_layer_sizes=[336, 96], dynedge_layer_sizes=[(128, 256), (336, 256)],
              global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)
    torch.manual_seed(9)
    ref = oracle.DynEdgeOracle(7, **kw)
    m = g.DynEdge(7, **kw)
    m.load_state_dict(ref.state_dict())
    m.to(DEV).set_backend(dtype=name)
    ei0 = oracle.knn_graph(b.x, 6, b.batch, [0, 1, 2, 3])
    b.edge_index = ei0
    y, trace = m(b.to(DEV), return_trace=True)
    assert y.shape == (b.x.shape[0], 96)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    bc = b.to("cpu")
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], ei0)
    coords = trace["knn_coords"][0].cpu()                                  # layer-2 graph: 9 neighbours, bit-exact
    assert torch.equal(forced[1], oracle.knn_graph(coords, 9, bc.batch, [0, 1, 2]))
    yo = ref(bc.x, ei0, bc.batch, bc.n_pulses, forced_edges=forced)
    (yo * w).sum().backward()
    assert rel_err(y, yo.detach()) < tol
    for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
        if po.grad is None:
            continue
        if mode == 0:
            assert rel_err(p.grad, po.grad) < 2e-3, f"{name}: grad {kn}"
        else:
            assert norm_err(p.grad, po.grad) < 5e-2, f"{name}: grad {kn}"


@pytest.mark.parametrize("name,mode,tol", MODES)
def test_particlenet_backbone(oracle, name, mode, tol):
    """ParticleNeT (models/gnn/particlenet.py): three-layer edge MLPs with BatchNorm1d over the edges of the batch
    (training: batch statistics + running-stat update; eval: running statistics), mean aggregation, 16 neighbours,
    re-clustering after every block (teacher-forced on the graphs the device built), mean pooling, read-out."""
    import graphnet_amd as g
    b = _batch(6, seed=57)
    b.x[3:25, :3] = b.x[2, :3]                  # > 17 pulses on one position: overflow rows with k = 16
    kw = dict(dynedge_layer_sizes=[(32, 32, 32), (64, 64, 64)], readout_layer_sizes=[48], dropout_readout=0.0)
    torch.manual_seed(12)
    ref = oracle.ParticleNeTOracle(7, **kw)
    m = g.ParticleNeT(7, **kw)
    assert list(m.state_dict()) == list(ref.state_dict())
    m.load_state_dict(ref.state_dict())
    m.to(DEV).set_backend(dtype=name)
    m.train(); ref.train()
    y, trace = m(b.to(DEV), return_trace=True)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    (y * w.to(DEV)).sum().backward()
    bc = b.to("cpu")
    forced = [t.edge_index().cpu() for t in trace["graphs"]]
    assert torch.equal(forced[0], oracle.knn_graph(bc.x, 16, bc.batch, [0, 1, 2]))
    yo = ref(bc.x, forced[0], bc.batch, bc.n_pulses, forced_edges=forced)
    (yo * w).sum().backward()
    assert rel_err(y, yo.detach()) < tol
    if mode == 0:   # the re-clustered graph is the oracle's k-NN of the same coordinates
        assert torch.equal(forced[1], oracle.knn_graph(trace["conv_out"][0].detach().cpu(), 16, bc.batch, [0, 1, 2]))
    # A Linear bias in front of a training-mode BatchNorm has an exactly-zero gradient (the batch mean absorbs it): both
    # sides hold rounding noise only (bf16: the cancellation of ~1e5 rounded terms of size 1e-2).  These parameters are
    # named by the structure of the network, not by the size of the oracle's noise, which depends on the host's CPU
    # and thread count.
    zero_grad = {f"_conv_layers.{l}.nn.{i}.bias" for l, conv in enumerate(ref._conv_layers)
                 for i, (a, nxt) in enumerate(zip(conv.nn, list(conv.nn)[1:]))
                 if isinstance(a, torch.nn.Linear) and isinstance(nxt, torch.nn.BatchNorm1d)}
    assert len(zero_grad) == 6
    for (kn, p), (_, po) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, kn
        if kn in zero_grad:
            print(f"{name}: zero-gradient {kn}: device max {float(p.grad.abs().max()):.3e}, oracle max {float(po.grad.abs().max()):.3e}")
            assert p.grad.abs().max() < (1e-5 if mode == 0 else 5e-3), kn
        elif mode == 0:
            assert rel_err(p.grad, po.grad) < 2e-3, f"{name}: grad {kn}"
        else:
            assert norm_err(p.grad, po.grad) < 8e-2, f"{name}: grad {kn}"
    sd, sdo = m.state_dict(), ref.state_dict()
    for k in sd:
        if "running" in k or "num_batches" in k:
            assert rel_err(sd[k].float(), sdo[k].float()) < (1e-4 if mode == 0 else 2e-2), k
    # eval mode: running statistics
    m.eval(); ref.eval()
    with torch.no_grad():
        ye, tre = m(b.to(DEV), return_trace=True)
        b.to("cpu")
        forced_e = [t.edge_index().cpu() for t in tre["graphs"]]      # eval-mode features give their own graphs
        yeo = ref(b.x, forced_e[0], b.batch, b.n_pulses, forced_edges=forced_e)
    assert rel_err(ye, yeo) < (2e-4 if mode == 0 else 3e-2)


@pytest.mark.parametrize("sizes", [[3, 0, 700, 1, 9000, 40, 2], [9000, 0, 12000, 3, 20000, 1]])
def test_event_local_reverse_build_equals_global_build(sizes):
    """gn_rev_build_events_ws (one workgroup per event / slice, LDS counters; scratch in HBM for slices above 8192 pulses; the
    second batch - few, huge events, N >= 2048 B - takes the bucketed build: rev_bucket_count / _scatter / _build)
    against gn_rev_build (global atomics): same offsets, same lists as sets, same hub nodes, hub lists sorted."""
    import copy
    from graphnet_amd import ops
    torch.manual_seed(0)
    assert (int(ops._lib.lib().gn_rev_pairs_ints(len(sizes), sum(sizes), 8)) > 0) == (sum(sizes) >= 2048 * len(sizes))
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    N = ptr[-1]
    x = torch.rand(N, 3)
    x[ptr[2]:ptr[2] + 300] = x[ptr[2]]                     # 300 pulses on one position: hubs + overflow rows
    x[ptr[4] + 100:ptr[4] + 180] = x[ptr[4] + 100]
    ptr_d = torch.tensor(ptr, dtype=torch.int32, device=DEV)
    batch = ops.ptr_to_batch(ptr_d, N)
    t = ops.knn_graph(x.to(DEV), [0, 1, 2], batch, ptr_d, 8)
    g = copy.copy(t)
    g.event_ptr = None
    t.build_reverse()
    g.build_reverse()
    assert t.rev_ptr is not g.rev_ptr
    assert torch.equal(t.rev_ptr, g.rev_ptr)
    rp = t.rev_ptr.cpu().numpy()
    a, b = t.rev_rows.cpu().numpy(), g.rev_rows.cpu().numpy()
    deg = np.diff(rp)
    assert deg.max() > 64
    for j in np.nonzero(deg)[0]:
        la, lb = a[rp[j]:rp[j + 1]], b[rp[j]:rp[j + 1]]
        assert sorted(la.tolist()) == sorted(lb.tolist()), j
        if deg[j] > 64:
            assert np.all(np.diff(la) > 0) and np.all(np.diff(lb) > 0)          # hub lists are sorted ascending
    na, nb_ = int(t.rev_nhubs[0]), int(g.rev_nhubs[0])
    assert na == nb_ == int((deg > 64).sum())
    assert sorted(t.rev_hubs[:na].cpu().tolist()) == sorted(g.rev_hubs[:nb_].cpu().tolist())


@pytest.mark.parametrize("case", ["k8_336", "k8_128", "k16_336", "k5_336_tiny", "hubs_336", "h340"])
def test_compact_dpre_is_bit_identical_to_the_dense_path(oracle, case):
    """csrc/dpre_compact.hip: the backward's edge-row tensor leaves the kernel without the elements its h-bits mark as
    zero and the source gather reads only the rest.  The same values are summed in the same order, so dP | dQ must equal
    the dense pair (``gn_edgeconv_bwd`` + ``gn_edgeconv_dq_gather``) BIT FOR BIT: table rows, (k+1)-th-neighbour overflow
    rows, hub sources (in-degree > 64: sorted lists, 16-wave kernel), 16-slot tables, tables with empty slots (k < 8 and
    events with fewer than k + 1 pulses), a last tile that is not full; and the planned tile sizes must add up to the
    number of set h-bits."""
    import ctypes
    from graphnet_amd import _lib, ops
    mode, dt, H2 = 1, torch.bfloat16, 256
    kk, H1, sizes = {"k8_336": (8, 336, None), "k8_128": (8, 128, None), "k16_336": (16, 336, None),
                     "k5_336_tiny": (5, 336, [1, 3, 2, 9, 70, 5]), "hubs_336": (8, 336, [400, 30]),
                     "h340": (8, 340, None)}[case]
    gen = torch.Generator().manual_seed(77)
    if sizes is None:
        b, x3, _, _, _ = _edgeconv_case(oracle, k=kk, F=32, H1=H1, H2=H2, n_events=40, seed=31)
        ptr32, batch32 = _csr(b)
        x3 = x3.clone()
    else:
        N = sum(sizes)
        x3 = torch.randn(N, 3, generator=gen)
        ptr32 = torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32).to(DEV)
        batch32 = torch.repeat_interleave(torch.arange(len(sizes), dtype=torch.int32), torch.tensor(sizes)).to(DEV)
    if case == "hubs_336":
        x3[5:200] = x3[5]            # 195 pulses at one position: the lowest ids among them collect > 64 in-edges each
    g = ops.knn_graph(x3.to(DEV), [0, 1, 2], batch32, ptr32, kk)
    N, H1p = g.N, ops.round_up(H1, 32)
    assert _lib.lib().gn_edgeconv_bwd_compact is not None          # (the path is opt-in for the model: GN_DPRE_COMPACT=1)
    PQ = (torch.randn(N, 2 * H1p, generator=gen) * 0.5).to(DEV).to(dt)
    PQ[:, H1:H1p] = 0
    PQ[:, H1p + H1:] = 0
    W2 = (torch.randn(H2, H1, generator=gen) * 0.1).to(DEV)
    b2 = (torch.randn(H2, generator=gen) * 0.1).to(DEV)
    W2p, W2Tp = ops.pack_weight(W2, [H1], dt), ops.pack_weight(W2.t().contiguous(), [H2], dt)
    gout = torch.randn(N, H2, generator=gen).to(DEV).to(dt)
    out, saved = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2, H2, H1=H1)
    ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, gout, saved)                    # writes the h-bits
    dense = torch.zeros(N, 2 * H1p, dtype=dt, device=DEV)
    dpre = torch.zeros(max(g.rows, 1), H1p, dtype=dt, device=DEV)
    ops.edgeconv_bwd(mode, g, PQ, H1p, H2, gout, saved, W2Tp, dpre, dense[:, :H1p])
    ops.edgeconv_dq_gather(mode, g, dpre, H1p, dense[:, H1p:])
    comp = torch.full((N, 2 * H1p), float("nan"), dtype=dt, device=DEV)
    ops.edgeconv_bwd_gather_compact(g, PQ, H1p, H1, H2, gout, saved, W2Tp, comp)
    torch.cuda.synchronize()
    if case == "hubs_336":
        deg = (g.rev_ptr[1:] - g.rev_ptr[:-1])
        assert int(deg.max()) > 64 and int(g.rev_nhubs[0]) > 0
    if case in ("k8_336", "hubs_336", "k16_336"):
        assert int(g.ovf_cnt.item()) > 0
    assert torch.equal(comp.view(torch.int16), dense.view(torch.int16)), \
        (case, float((comp.float() - dense.float()).abs().max()))
    # the plan: tile sizes = set h-bits of the tile's valid rows (16-byte units, rounded up); halves the dense bytes
    L = _lib.lib()
    plan = torch.empty(int(L.gn_edgeconv_dpre_plan_bytes(N, kk)), dtype=torch.uint8, device=DEV)
    _lib.check(L.gn_edgeconv_dpre_plan(N, kk, H1p, H1, H2, saved.data_ptr(), plan.data_ptr(), ops._st()))
    offs = (ctypes.c_int64 * 3)()
    L.gn_edgeconv_saved_offsets(N, kk, H1p, H2, ctypes.cast(offs, ctypes.c_void_p))
    S = g.S
    tiles = (N * S + 63) // 64
    hb = saved[int(offs[2]): int(offs[2]) + tiles * 64 * (H1p // 8)].cpu().numpy().reshape(tiles * 64, H1p // 8)
    import numpy as np
    bits = np.unpackbits(hb, axis=1, bitorder="little")[:, :(H1 + 7) // 8 * 8]
    rows = np.arange(tiles * 64)
    valid = (rows < N * S) & ((rows % S) < kk)
    nnz = (bits.sum(1) * valid).reshape(tiles, 64).sum(1)
    up256 = lambda v: (v + 255) // 256 * 256
    ts = plan[up256(tiles * 128): up256(tiles * 128) + 4 * tiles].view(torch.int32).cpu().numpy()
    assert np.array_equal(ts, (nnz * 2 + 15) // 16)
    if sizes is None:
        assert 0.3 < nnz.sum() / (valid.sum() * H1) < 0.7          # about half of dpre is zeros the h-bits mark


def test_generic_dynedge_lean_backward_is_bit_identical(monkeypatch):
    """GELU / LayerNorm DynEdge (csrc/generic.hip path): with GN_GENERIC_LEAN=1 the three edge-row tensors of every layer
    are rebuilt in the backward from P|Q instead of kept from the forward - same kernels on the same inputs, so output and
    every gradient must be bit for bit those of the keeping mode (the mode large batches fall into by themselves)."""
    import graphnet_amd as g
    b = _batch(9, seed=31)
    kw = dict(nb_neighbours=9, post_processing_layer_sizes=[336, 96], dynedge_layer_sizes=[(128, 256), (336, 256)],
              global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)
    res = {}
    for lean in ("0", "1"):
        monkeypatch.setenv("GN_GENERIC_LEAN", lean)
        torch.manual_seed(4)
        m = g.DynEdge(7, **kw).to(DEV)
        m.set_backend(dtype="bf16")
        y = m(b.to(DEV))
        w = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
        (y * w).sum().backward()
        res[lean] = (y.detach().clone(), [p.grad.clone() for p in m.parameters() if p.grad is not None])
        b = b.to("cpu")
    assert torch.equal(res["0"][0], res["1"][0])
    assert len(res["0"][1]) == len(res["1"][1]) > 0
    for a, c in zip(res["0"][1], res["1"][1]):
        assert torch.equal(a, c)


@pytest.mark.parametrize("k", [9, 8, 5])
def test_generic_dynedge_on_compact_rows(monkeypatch, k):
    """The unfused GELU / LayerNorm path on the EXISTING edges only (``gn_rows_compact``: N k + overflow rows instead of the
    slot layout's 17 N for k = 9): every row of the forward is computed by the same arithmetic and a centre's rows are
    summed in the same order, so the OUTPUT is bit for bit the slot layout's; weight gradients are sums over all rows in
    another grouping (equal to rounding), input-side gradients go through the rewritten reverse lists."""
    import graphnet_amd as g
    b = _batch(9, seed=33)
    b.x[5:5 + k + 4, :3] = b.x[4, :3]                               # > k coincident pulses: overflow rows
    kw = dict(nb_neighbours=k, post_processing_layer_sizes=[336, 96], dynedge_layer_sizes=[(128, 256), (336, 256)],
              global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)
    res = {}
    for compact in ("0", "1"):
        monkeypatch.setenv("GN_GENERIC_COMPACT", compact)
        torch.manual_seed(4)
        m = g.DynEdge(7, **kw).to(DEV)
        m.set_backend(dtype="fp32")
        y, trace = m(b.to(DEV), return_trace=True)
        w = torch.randn(y.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
        (y * w).sum().backward()
        res[compact] = (y.detach().clone(), [p.grad.clone() for p in m.parameters() if p.grad is not None],
                        int(trace["graphs"][0].ovf_cnt.item()))
        b = b.to("cpu")
    assert res["1"][2] > 0
    assert torch.equal(res["0"][0], res["1"][0])
    for a, c in zip(res["0"][1], res["1"][1]):
        assert norm_err(c, a) < 1e-5
