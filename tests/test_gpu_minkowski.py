"""``gn_minkowski_knn_graph`` / ``MinkowskiKNNEdges`` on the device against ``oracle.minkowski_knn``
(oracle/knn_oracle.c:105-146, pinned on the reference's own known answer by tests/test_oracle_pins.py).

Every comparison is exact (``torch.equal``): the arithmetic is specified operation by operation and the selection is the
total order ``(m, j)``, so there is nothing to tolerate.  The oracle runs per event on
``x[:, space_coords + [time_coord]]`` (two space columns: a zero column is added, ``+ 0.0`` is exact) and its edge list is
laid out as the strict table, ``-1`` padded to ``k``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ptr_of(sizes):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
    return ptr


def _oracle_table(oracle, x, ptr, k, c, tlw=1.0, space=(0, 1, 2), time=3):
    """Expected ``nbr[N, k]`` (int32, -1 padded) of a CPU ``x`` with event offsets ``ptr``."""
    x = x.detach().to(torch.float32).cpu()
    N = int(x.shape[0])
    nbr = torch.full((N, k), -1, dtype=torch.int32)
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        if hi - lo < 1:
            continue
        cols = [x[lo:hi, s] for s in space]
        if len(cols) == 2:
            cols.append(torch.zeros(hi - lo))
        assert len(cols) == 3
        sub = torch.stack(cols + [x[lo:hi, time]], dim=1).contiguous()
        ei, _ = oracle.minkowski_knn(sub, k, c, tlw)
        src, dst = ei[0], ei[1]                                   # grouped by centre, ascending (m, j) inside a group
        slot = np.arange(len(dst)) - np.searchsorted(dst, dst, side="left")
        nbr[lo + torch.from_numpy(dst), torch.from_numpy(slot)] = torch.from_numpy(src + lo).to(torch.int32)
    return nbr


def _edge_index_of(nbr):
    n, w = nbr.shape
    centre = torch.arange(n, dtype=torch.int64).unsqueeze(1).expand(n, w)
    valid = nbr >= 0
    return torch.stack([nbr[valid].to(torch.int64), centre[valid]], dim=0)


def _device_table(x, ptr, k, c, tlw=1.0, space=(0, 1, 2), time=3):
    from graphnet_amd import ops
    ptr32 = ptr.to(torch.int32).to(DEV)
    batch32 = ops.ptr_to_batch(ptr32, int(x.shape[0]))
    t = ops.minkowski_knn_graph(x, list(space), time, c, tlw, batch32, ptr32, k)
    assert t.ovf is None and t.K == k and tuple(t.nbr.shape) == (int(x.shape[0]), k)     # the strict form
    return t


# ------------------------------------------------------------------------------ 1. the reference's known answer
def test_reference_known_answer(oracle, golden):
    ka = golden["reference_known_answers"]                     # tests/models/test_minkowski.py:104-160 of the reference
    x = torch.from_numpy(ka["minkowski_vec1"]).to(torch.float32)
    exp = ka["minkowski_knn_k2_edge_index"]
    ptr = _ptr_of([x.shape[0]])
    t = _device_table(x.to(DEV), ptr, 2, 1.0)
    ei = t.edge_index().cpu().numpy()
    assert np.array_equal(ei[1], exp[1])
    for i in range(x.shape[0]):                                # the oracle pin's criterion: sources per centre, as sets
        assert set(ei[0][ei[1] == i].tolist()) == set(exp[0][exp[1] == i].tolist())
    assert torch.equal(t.nbr.cpu(), _oracle_table(oracle, x, ptr, 2, 1.0))


# ------------------------------------------------------------------------------ 2. tile / chunk / split boundaries
SIZES = [1, 2, 3, 9, 63, 64, 65, 256, 257, 600]


@pytest.fixture(scope="module")
def shapes_batch():
    gen = torch.Generator().manual_seed(20)
    n = sum(SIZES)
    x = torch.cat([torch.randn(n, 3, generator=gen), torch.rand(n, 1, generator=gen) * 3.0], dim=1).contiguous()
    return x, _ptr_of(SIZES), x.to(DEV)


@pytest.mark.parametrize("tlw", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("c", [0.3, 1.0])
@pytest.mark.parametrize("k", [2, 8, 16, 24, 32])
def test_shapes_where_the_kernel_can_go_wrong(oracle, shapes_batch, k, c, tlw):
    x, ptr, xd = shapes_batch
    t = _device_table(xd, ptr, k, c, tlw)
    exp = _oracle_table(oracle, x, ptr, k, c, tlw)
    assert torch.equal(t.nbr.cpu(), exp)
    deg = (t.nbr >= 0).sum(1).cpu()                            # degree min(k, n - 1), also where n <= k
    n_of = torch.repeat_interleave(torch.tensor(SIZES), torch.tensor(SIZES))
    assert torch.equal(deg, torch.clamp(n_of - 1, max=k))


# ------------------------------------------------------------------------------ 3. ties, NaN / inf, raw scale
@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("c", [1.0, 0.5])
def test_ties_on_an_integer_grid(oracle, k, c):
    gen = torch.Generator().manual_seed(5)
    sizes = [300, 90]
    n = sum(sizes)
    x = torch.cat([torch.randint(0, 4, (n, 3), generator=gen), torch.randint(0, 5, (n, 1), generator=gen)], 1).float()
    x[40:60] = x[40]                                           # twenty coincident pulses: more than k + 1 where k = 8, 16
    x[7, 1] = float("nan")
    x[11, 3] = float("inf")
    ptr = _ptr_of(sizes)
    t = _device_table(x.to(DEV), ptr, k, c, 2.0)
    got = t.nbr.cpu()
    assert torch.equal(got, _oracle_table(oracle, x, ptr, k, c, 2.0))
    for bad in (7, 11):                                        # no neighbours, nobody's neighbour
        assert bool((got[bad] == -1).all()) and not bool((got == bad).any())
    assert bool((got[40:60] >= 0).all())                       # m == 0 ties with the centre itself: excluded by index
    assert not bool((got == torch.arange(n, dtype=torch.int32).unsqueeze(1)).any())


def test_raw_scale_distances_above_1e10(oracle):
    """Raw detector units: metres, nanoseconds, c = 0.3 m/ns.  Pulses 1 ms apart sit at m ~ 9e10 and more, above the
    Euclidean path's 1e10 sentinel: they are still neighbours."""
    gen = torch.Generator().manual_seed(9)
    sizes = [12, 70]
    n = sum(sizes)
    x = torch.cat([torch.rand(n, 3, generator=gen) * 1000.0 - 500.0, torch.zeros(n, 1)], 1)
    x[:, 3] = 1.0e4 + torch.arange(n, dtype=torch.float32) * 1.0e6
    ptr = _ptr_of(sizes)
    t = _device_table(x.to(DEV), ptr, 8, 0.3, 1.0)
    assert torch.equal(t.nbr.cpu(), _oracle_table(oracle, x, ptr, 8, 0.3, 1.0))
    assert bool((t.nbr >= 0).all())                            # degree 8 = min(k, n - 1) everywhere


# ------------------------------------------------------------------------------ 4. columns and row pitch
@pytest.mark.parametrize("case", ["permuted", "two_space", "strided"])
def test_columns_and_row_pitch(oracle, case):
    gen = torch.Generator().manual_seed(31)
    sizes = [5, 130, 70, 300]
    n = sum(sizes)
    ptr = _ptr_of(sizes)
    x = torch.randn(n, 7, generator=gen)
    space, time, xd = [4, 0, 2], 5, None
    if case == "two_space":
        space, time = [6, 1], 0
    if case == "strided":
        big = torch.randn(n, 12, generator=gen).to(DEV)
        xd = big[:, 3:10]                                      # row pitch 12, seven columns, not contiguous
        assert not xd.is_contiguous()
        x = xd.cpu().contiguous()
    else:
        xd = x.to(DEV)
    t = _device_table(xd, ptr, 8, 0.7, 1.5, space, time)
    assert torch.equal(t.nbr.cpu(), _oracle_table(oracle, x, ptr, 8, 0.7, 1.5, space, time))


# ------------------------------------------------------------------------------ 5. whole-event scan of large events
def test_large_events_are_scanned_whole_by_one_wave(oracle):
    """50 events of 1000 pulses: 800 tiles of events above 256 pulses, at least the 768 from which one wave scans its whole
    event (four LDS chunks) instead of eight waves sharing it; and events of this size never take the sorted sweep."""
    gen = torch.Generator().manual_seed(77)
    sizes = [1000] * 50
    n = sum(sizes)
    x = torch.cat([torch.randn(n, 3, generator=gen), torch.rand(n, 1, generator=gen) * 2.0], dim=1).contiguous()
    ptr = _ptr_of(sizes)
    t = _device_table(x.to(DEV), ptr, 8, 1.0, 1.0)
    assert torch.equal(t.nbr.cpu(), _oracle_table(oracle, x, ptr, 8, 1.0, 1.0))


# ------------------------------------------------------------------------------ 6. the edge definition on device
def test_edge_definition_on_a_device_batch_and_on_a_single_event(oracle):
    import graphnet_amd as g
    from graphnet_amd.synthetic import synthetic_icecube86_batch
    b = synthetic_icecube86_batch(6, seed=17)
    x, ptr = b.x.clone(), b.ptr.clone()
    ed = g.MinkowskiKNNEdges(8, c=18.0, time_like_weight=0.5)
    out = ed(b.to(DEV))
    assert out.edge_index.is_cuda and out.edge_index.dtype == torch.int64
    assert torch.equal(out.edge_index.cpu(), _edge_index_of(_oracle_table(oracle, x, ptr, 8, 18.0, 0.5)))
    lo, hi = int(ptr[2]), int(ptr[3])
    one = ed(g.Data(x=x[lo:hi].to(DEV)))                       # no `batch`: one event
    exp = _edge_index_of(_oracle_table(oracle, x[lo:hi], _ptr_of([hi - lo]), 8, 18.0, 0.5))
    assert torch.equal(one.edge_index.cpu(), exp)


# ------------------------------------------------------------------------------ 7. the backbone honours the record
def _strip_record(b):
    from graphnet_amd.graphs import MINKOWSKI_RECORD
    for name in MINKOWSKI_RECORD:
        b[name] = None
    return b


@pytest.mark.parametrize("path", ["collate", "batch_from_raw"])
def test_dynedge_builds_the_recorded_graph(oracle, path):
    import graphnet_amd as g
    from graphnet_amd.graphs import minkowski_record
    from graphnet_amd.synthetic import FEATURES_ICECUBE86, synthetic_icecube86_raw
    k, c, tlw = 8, 18.0, 2.0
    raw, rptr, _ = synthetic_icecube86_raw(6, seed=23)
    events = [raw[rptr[i]:rptr[i + 1]].astype(np.float64) for i in range(6)]
    gd = g.GraphDefinition(g.IceCube86(), input_feature_names=FEATURES_ICECUBE86,
                           edge_definition=g.MinkowskiKNNEdges(k, c=c, time_like_weight=tlw))
    if path == "collate":
        b = g.collate_fn([gd(e, FEATURES_ICECUBE86) for e in events])      # on the CPU: no edges, the record
        assert "edge_index" not in b.keys()
        b = b.to(DEV)
    else:
        b = gd.batch_from_raw(events, FEATURES_ICECUBE86, device=DEV)
    assert minkowski_record(b) == (k, c, tlw, 3, [0, 1, 2])
    exp_ei = _edge_index_of(_oracle_table(oracle, b.x.cpu(), b.ptr.cpu(), k, c, tlw))

    torch.manual_seed(4)
    # pooled output: without pooling schemes a DynEdge has no one-call path at all
    m = g.DynEdge(7, dynedge_layer_sizes=[(128, 256), (336, 256)],
                  global_pooling_schemes=["min", "max", "mean", "sum"]).to(DEV)
    m.set_backend(dtype="fp32")
    assert m._stepper(7) is not None                                        # this configuration takes the one-call path
    with torch.no_grad():
        out_step = m(b)                                                     # the one-call path
        out_trace, trace = m(b, return_trace=True)                          # the per-op path
        assert torch.equal(trace["graphs"][0].edge_index().cpu(), exp_ei)
        explicit = g.Batch(x=b.x, edge_index=exp_ei.to(DEV))
        explicit.ptr, explicit.batch, explicit.n_pulses = b.ptr, b.batch, b.n_pulses
        assert minkowski_record(explicit) is None
        ref_step = m(explicit)
        ref_trace, _ = m(explicit, return_trace=True)
    assert torch.equal(out_step, ref_step) and torch.equal(out_trace, ref_trace)
    assert torch.equal(out_step, ref_trace)
    # and it is not the Euclidean graph that was built
    with torch.no_grad():
        assert not torch.equal(m(_strip_record(b)), out_step)
