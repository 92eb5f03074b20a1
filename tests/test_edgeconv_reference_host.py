"""CPU: the reference that ``tests/test_gpu_edgeconv_relu.py`` holds the ReLU edge-convolution kernels to
(``tests/edgeconv_reference.py``) is itself right, and its lattice cases cannot pass vacuously.

(a) on real-valued float64 inputs its explicit formulas equal torch autograd through a plain gather, two Linear layers
    with ReLU and ``index_add``, to 1e-12, on a small hand-made table with empty slots, an overflow row and an isolated
    node;
(b) on lattice inputs the fp32 evaluation with the hidden columns and the edge rows in a shuffled order equals the float64
    one EXACTLY (so the float64 result is the one correct fp32 answer, whatever order a kernel sums in), and
    ``mirror_bf16`` changes nothing but roundings;
(c) every (shape, seed) of the GPU test, on the graph of its crafted batch (the C oracle's k-NN table, which the device
    table equals bit for bit - ``test_gpu_kernels.py::test_knn_bit_exact_synthetic``): open gates within [0.3, 0.7] at
    both layers, exact zeros at both, max|dW2| * 32 < 2^24, and the graph features the batch was crafted for."""
import pytest
import torch

import edgeconv_reference as er


def _hand_made():
    # 6 nodes, K = 3, S = 4 (a table wider than K: slot 3 is always empty).  Node 4 is isolated (no edge in or out);
    # node 0 has a full row AND an overflow row; node 2 has one edge; node 5 is a source only
    nbr = torch.tensor([[1, 2, 3], [0, 2, -1], [5, -1, -1], [0, 1, 2], [-1, -1, -1], [-1, -1, -1]])
    return er.HostGraph(nbr, torch.tensor([0]), torch.tensor([5]), 3, 4)


def test_reference_equals_autograd_on_a_hand_made_table():
    g = _hand_made()
    f = g.features()
    assert f["ovf_cnt"] == 1 and f["centres_without_edge"] == 2 and f["sources_without_in_edge"] == 1 and f["empty_slots"] == 9
    N, H1, H1p, H2 = g.N, 5, 8, 7
    gen = torch.Generator().manual_seed(3)
    PQ = torch.randn(N, 2 * H1p, generator=gen, dtype=torch.float64)
    PQ[:, H1:H1p] = 0
    PQ[:, H1p + H1:] = 0
    W2 = torch.randn(H2, H1, generator=gen, dtype=torch.float64)
    b2 = torch.randn(H2, generator=gen, dtype=torch.float64)
    gout = torch.randn(N, H2, generator=gen, dtype=torch.float64)
    ref = er.reference(g, PQ, H1p, H1, W2, b2, gout, coord_cols=(0, 2))
    # autograd: gather, Linear + ReLU twice (the first Linear is the P | Q split), index_add; edges listed by hand
    src = torch.tensor([1, 2, 3, 0, 2, 5, 0, 1, 2, 5])
    dst = torch.tensor([0, 0, 0, 1, 1, 2, 3, 3, 3, 0])
    row = torch.tensor([0, 1, 2, 4, 5, 8, 12, 13, 14, 24])             # i * S + s; the overflow row is N * S + 0
    PQa, W2a, b2a = PQ.clone().requires_grad_(), W2.clone().requires_grad_(), b2.clone().requires_grad_()
    pre1 = PQa[dst, :H1] + PQa[src, H1p:H1p + H1]
    pre1.retain_grad()
    out = torch.zeros(N, H2, dtype=torch.float64).index_add(0, dst, torch.relu(torch.relu(pre1) @ W2a.t() + b2a))
    (out * gout).sum().backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(ref.out, out.detach()) and close(ref.coords, out.detach()[:, [0, 2]])
    assert close(ref.dW2, W2a.grad) and close(ref.db2, b2a.grad)
    assert close(ref.dP, PQa.grad[:, :H1p]) and close(ref.dQ, PQa.grad[:, H1p:])
    dpre = torch.zeros(g.nrows, H1p, dtype=torch.float64)
    dpre[row, :H1] = pre1.grad
    assert ref.dpre.shape == (N * 4 + 1, H1p) and close(ref.dpre, dpre)
    assert float(ref.dP[:, H1:].abs().max()) == 0 and float(ref.dQ[:, H1:].abs().max()) == 0
    assert float(ref.out[4].abs().max()) == 0 and float(ref.dQ[4].abs().max()) == 0 and float(ref.dP[5].abs().max()) == 0


@pytest.fixture(scope="module")
def oracle_graphs(oracle):
    def build(k, strict):
        x, ptr = er.batch_coords(k)
        tab, _ = oracle.knn_table(x, k, ptr, [0, 1, 2], "strict" if strict else "compat")
        return er.HostGraph.from_oracle_table(tab, k)
    cache = {}
    return lambda k, strict: cache.setdefault((k, strict), build(k, strict))


def test_lattice_float32_in_any_order_is_the_float64_result(oracle_graphs):
    # the shape the idea was checked at: N = 195, K = 8, H1 = 336, H2 = 256
    g = oracle_graphs(8, False)
    H1, H1p, H2 = 336, 352, 256
    PQ, W2, b2, gout = er.lattice_inputs(g.N, H1, H1p, H2)
    for t, lim, unit in ((PQ, 2, 8), (W2, 1, 8), (b2, 1, 8), (gout, 2, 4)):
        assert float(t.abs().max()) <= lim and torch.equal(t * unit, (t * unit).round())
        assert torch.equal(t.bfloat16().float(), t)                    # a bf16 number: the bf16 kernels see the same operands
    assert float(PQ[:, H1:H1p].abs().max()) == 0 and float(PQ[:, H1p + H1:].abs().max()) == 0
    ref = er.reference(g, PQ, H1p, H1, W2, b2, gout)
    gen = torch.Generator().manual_seed(1)
    E = int(g.rows()[0].shape[0])
    f32 = er.reference(g, PQ, H1p, H1, W2, b2, gout, dtype=torch.float32, col_perm=torch.randperm(H1, generator=gen),
                       edge_perm=torch.randperm(E, generator=gen))
    for key in ("out", "coords", "dW2", "db2", "dpre", "dP", "dQ"):
        assert torch.equal(getattr(f32, key).double(), getattr(ref, key)), key
    assert (f32.zeros1, f32.zeros2) == (ref.zeros1, ref.zeros2)
    # lowp (the bf16 mode's operand roundings) is the identity on the lattice
    low = er.reference(g, PQ, H1p, H1, W2, b2, gout, lowp=True)
    for key in ("out", "dW2", "db2", "dpre", "dP", "dQ"):
        assert torch.equal(getattr(low, key), getattr(ref, key)), key


@pytest.mark.parametrize("table,ovf", [("tiled", "tiled"), ("persistent", "gemm"), ("persistent", "tiled")])
def test_mirror_only_rounds(oracle_graphs, table, ovf):
    g = oracle_graphs(8, False)
    H1, H1p, H2 = 128, 128, 256
    PQ, W2, b2, gout = er.lattice_inputs(g.N, H1, H1p, H2)
    ref = er.reference(g, PQ, H1p, H1, W2, b2, gout)
    mir = er.mirror_bf16(g, ref, H1p, table, ovf)
    u = 2.0 ** -8                                                      # unit roundoff of bf16 (8 significant bits, RNE)
    for key, roundings in (("out", 3), ("dpre", 1), ("dP", 4), ("dQ", 2)):
        a, b = getattr(mir, key), getattr(ref, key)
        assert torch.equal(a.float().bfloat16().double(), a), key     # every value is a bf16 number
        assert not torch.equal(a, b), key                              # ... and the rounding does bite at these sizes
        scale = {"out": ref.out.abs(), "dpre": ref.dpre.abs(),
                 "dP": torch.zeros_like(ref.dP).index_add(0, ref.c, torch.nn.functional.pad(ref.d.abs(), (0, H1p - H1))),
                 "dQ": torch.zeros_like(ref.dQ).index_add(0, ref.s, torch.nn.functional.pad(ref.d.abs(), (0, H1p - H1)))}[key]
        assert bool(((a - b).abs() <= roundings * u * scale * (1 + u) ** roundings).all()), key
    # centres without an overflow row: coords are the exact fp32 slot sums on every path
    plain = torch.ones(g.N, dtype=torch.bool)
    plain[g.ovf_centre] = False
    assert torch.equal(mir.coords[plain], ref.coords[plain])
    assert torch.equal(mir.coords, ref.coords) == (ovf == "tiled")


@pytest.mark.parametrize("case", er.CASES, ids=er.case_id)
def test_lattice_cases_are_not_vacuous(oracle_graphs, case):
    k, H1, H2, strict = case
    g = oracle_graphs(k, strict)
    f = g.features()
    assert f["n_mod_8"] != 0 and f["partial_last_tile"]
    assert f["centres_without_edge"] >= 1 and f["sources_without_in_edge"] >= 1 and f["empty_slots"] >= 1
    assert f["max_in_degree"] > 64                                     # hub sources (the 16-wave gather kernel)
    assert (f["ovf_cnt"] == 0) if strict else (f["ovf_cnt"] > 0)
    H1p = er.round_up(H1, 32)
    ref = er.reference(g, *_split(er.lattice_inputs(g.N, H1, H1p, H2), H1p, H1))
    assert er.lattice_conditions(ref) == [], (case, er.lattice_conditions(ref))


def _split(inputs, H1p, H1):
    PQ, W2, b2, gout = inputs
    return PQ, H1p, H1, W2, b2, gout
