"""Plain torch reference of the fused ReLU edge convolution (``gn_edgeconv_fwd / _dw2 / _bwd / _dq_gather``), evaluated
on the CPU from HOST COPIES OF THE NEIGHBOUR TABLE'S FIELDS (``nbr``, ``ovf_centre``, ``ovf_src``, ``ovf_cnt``, K, S) in the
kernels' own edge-row layout - not through ``edge_index()``, which is device code of its own::

    table row  i * S + s   centre i, source nbr[i, s]         (s < K and nbr[i, s] >= 0, else the row is EMPTY: all 0)
    overflow   N * S + q   centre ovf_centre[q], source ovf_src[q]        (q < ovf_cnt)

    pre1 = P[c] + Q[s]        h = relu(pre1)        z2 = h W2^T + b2        m = relu(z2)        out[c] += m
    dm = g_out[c] [z2 > 0]    dW2 = dm^T h          db2 = colsum(dm)
    dpre = (dm W2) [pre1 > 0]                       dP[c] += dpre           dQ[s] += dpre

(both gates strict, as torch's relu backward and the kernels, edgeconv.hip:158-159, 311-312).

Lattice inputs (:func:`lattice_inputs`): P, Q, W2, b2 multiples of 1/8 (|P|, |Q| <= 2, |W2|, |b2| <= 1), g_out multiples of
1/4 (|g_out| <= 2).  Every operand is then a bf16 AND an fp32 number, every product and every partial sum of the three
passes is an fp32 number in any summation order (h: 6 bits; z2: multiples of 1/64 below 2^11; dm W2: multiples of 1/32
below 2^10; dW2: below 2^24 units of 1/32 up to 65 536 edge rows), so every relu decision - exact zeros included - is the
same in every kernel family and in float64, and the float64 result IS the correct fp32 result: a missing, doubled or
misrouted term is an inequality, not a tolerance question.  ``tests/test_edgeconv_reference_host.py`` checks all of this
on the CPU.

:func:`mirror_bf16` applies the bf16 roundings of the bf16 kernels at the points where the kernels round; the points
differ between the kernel families (see there).  No test in this module."""
from types import SimpleNamespace

import torch

SIZES = (1, 3, 2, 9, 70, 110)          # pulses per event of the one batch all shapes share: 195 in all
# (k, H1, H2): the smallest shapes at which the kernels branch (tests/test_gpu_edgeconv_relu.py lists why each is here)
SHAPES = [(8, 336, 256), (8, 128, 256), (16, 336, 256), (12, 128, 256), (8, 340, 256), (8, 348, 256), (5, 100, 96)]
# (k, H1, H2, strict); the last one has no overflow list at all
CASES = [(k, h1, h2, False) for (k, h1, h2) in SHAPES] + [(8, 336, 256, True)]
COORD_COLS = (0, 1, 2, 5)
LATTICE_SEED = 7


def case_id(case):
    k, h1, h2, strict = case
    return f"k{k}_h{h1}_o{h2}" + ("_strict" if strict else "")


def round_up(v, m):
    return (v + m - 1) // m * m


def slots(K):
    return 8 if K <= 8 else (16 if K <= 16 else 32)


# ------------------------------------------------------------------------------------------------------------- graph
def batch_coords(k):
    """Crafted coordinates ``x[195, 3]`` (fp32) and the event offsets ``ptr`` of :data:`SIZES`: ``k + 6`` pulses of the
    70-pulse event share a position ((k+1)-th neighbours: overflow rows), 80 pulses of the 110-pulse event share one (the
    lowest ids among them collect more than 64 in-edges: hub sources); events of 1, 3 and 2 pulses give a centre without
    an edge, sources without an in-edge and empty slots.  195 is no multiple of 8 and 195 * S no multiple of 64."""
    ptr = torch.zeros(len(SIZES) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor(SIZES), 0)
    x = torch.randn(int(ptr[-1]), 3, generator=torch.Generator().manual_seed(2024))
    e4, e5 = int(ptr[4]), int(ptr[5])
    x[e4 + 3: e4 + 3 + k + 6] = x[e4 + 2]
    x[e5 + 5: e5 + 85] = x[e5 + 5]
    return x, ptr


class HostGraph:
    """Host copy of a neighbour table.  ``nbr`` [N, K] (-1 = no edge), ``ovf_centre`` / ``ovf_src`` [cnt]."""

    def __init__(self, nbr, ovf_centre, ovf_src, K, S):
        self.nbr = nbr.to(torch.int64).cpu()
        self.N, self.K, self.S = int(nbr.shape[0]), int(K), int(S)
        assert self.nbr.shape[1] == self.K and self.S >= self.K
        none = torch.zeros(0, dtype=torch.int64)
        self.ovf_centre = none if ovf_centre is None else ovf_centre.to(torch.int64).cpu()
        self.ovf_src = none if ovf_src is None else ovf_src.to(torch.int64).cpu()
        self.cnt = int(self.ovf_centre.shape[0])
        assert self.ovf_centre.unique().numel() == self.cnt            # at most one overflow row per centre
        self.nrows = self.N * self.S + self.cnt                        # rows a backward kernel must write

    @classmethod
    def from_table(cls, g):
        """From the device fields of an ``ops.NeighbourTable`` (one read-back of the overflow count)."""
        if g.ovf_cnt is None:
            return cls(g.nbr, None, None, g.K, g.S)
        cnt = int(g.ovf_cnt.item())
        return cls(g.nbr, g.ovf_centre[:cnt], g.ovf_src[:cnt], g.K, g.S)

    @classmethod
    def from_oracle_table(cls, tab, K):
        """From the C oracle's ``knn_table`` [N, K + 1]: column K is the (K+1)-th neighbour, listed by ascending centre."""
        tab = tab.to(torch.int64)
        centre = torch.nonzero(tab[:, K] >= 0).flatten()
        return cls(tab[:, :K], centre, tab[centre, K], K, slots(K))

    def rows(self):
        """``(row id, centre, source)`` of the rows that are edges: table rows in row order, then the overflow rows."""
        i, s = torch.nonzero(self.nbr >= 0, as_tuple=True)
        row = torch.cat([i * self.S + s, self.N * self.S + torch.arange(self.cnt)])
        return row, torch.cat([i, self.ovf_centre]), torch.cat([self.nbr[i, s], self.ovf_src])

    def features(self):
        """What the crafted batch is meant to contain (the tests assert it rather than assume it)."""
        _, c, s = self.rows()
        deg_in = torch.bincount(s, minlength=self.N)
        return dict(ovf_cnt=self.cnt, max_in_degree=int(deg_in.max()) if self.N else 0,
                    centres_without_edge=int((torch.bincount(c, minlength=self.N) == 0).sum()),
                    sources_without_in_edge=int((deg_in == 0).sum()), empty_slots=int((self.nbr < 0).sum()),
                    partial_last_tile=(self.N * self.S) % 64 != 0, n_mod_8=self.N % 8)


# ------------------------------------------------------------------------------------------------------------ inputs
def lattice_inputs(N, H1, H1p, H2, seed=LATTICE_SEED):
    """``(PQ [N, 2 H1p], W2 [H2, H1], b2 [H2], gout [N, H2])`` fp32 on the dyadic lattice of the module docstring; the pad
    columns H1..H1p-1 of P and of Q are 0."""
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)
    PQ = torch.zeros(N, 2 * H1p)
    PQ[:, :H1] = ri(-16, 16, (N, H1)) / 8
    PQ[:, H1p:H1p + H1] = ri(-16, 16, (N, H1)) / 8
    return PQ, ri(-8, 8, (H2, H1)) / 8, ri(-8, 8, (H2,)) / 8, ri(-8, 8, (N, H2)) / 4


def real_inputs(N, k, H1, H1p, H2, act_dtype):
    """The generator of ``test_gpu_leaky.py::test_leaky_edgeconv_against_autograd``: P|Q and g_out are values of the
    mode's activation type, W2 and b2 fp32."""
    gen = torch.Generator().manual_seed(11 + k + H1)
    PQ = (torch.randn(N, 2 * H1p, generator=gen) * 0.7).to(act_dtype)
    PQ[:, H1:H1p] = 0
    PQ[:, H1p + H1:] = 0
    W2 = torch.randn(H2, H1, generator=gen) * 0.1
    b2 = torch.randn(H2, generator=gen) * 0.1
    gout = torch.randn(N, H2, generator=gen).to(act_dtype)
    return PQ, W2, b2, gout


# --------------------------------------------------------------------------------------------------------- reference
def reference(g, PQ, H1p, H1, W2, b2, gout, coord_cols=COORD_COLS, dtype=torch.float64, lowp=False, col_perm=None,
              edge_perm=None):
    """The three passes in ``dtype`` on the CPU.  ``lowp`` (bf16 mode on real-valued inputs): W2 is the bf16 operand the
    kernels see and the hidden activation enters the second layer and dW2 rounded to bf16, straight-through for the
    gradient (``test_gpu_leaky.py::_reference``; on lattice inputs both roundings are the identity).  ``col_perm`` /
    ``edge_perm``: evaluate with the H1 hidden columns / the edge rows in that order (summation-order checks).

    Returns a namespace: ``out`` [N, H2], ``coords`` [N, len(coord_cols)], ``dW2`` [H2, H1], ``db2`` [H2], ``dpre``
    [N * S + cnt, H1p] (empty slots 0), ``dP`` / ``dQ`` [N, H1p] (pad columns 0), the shares of open gates ``open1`` /
    ``open2`` and the numbers of pre-activations that are exactly 0, ``zeros1`` / ``zeros2``; and for
    :func:`mirror_bf16` the edge rows ``row, c, s`` with their messages ``m`` [E, H2] and ``d`` = dpre rows [E, H1]."""
    N, H2 = g.N, int(W2.shape[0])
    cv = lambda t: t.detach().cpu().to(dtype)
    PQ, b2, gout = cv(PQ), cv(b2), cv(gout)
    W2 = cv(W2.detach().cpu().float().bfloat16()) if lowp else cv(W2)
    row, c, s = g.rows()
    if edge_perm is not None:
        row, c, s = row[edge_perm], c[edge_perm], s[edge_perm]
    cp = torch.arange(H1) if col_perm is None else col_perm
    P, Q, W = PQ[:, :H1][:, cp], PQ[:, H1p:H1p + H1][:, cp], W2[:, cp]
    zero = torch.zeros((), dtype=dtype)
    pre1 = P[c] + Q[s]
    h = torch.where(pre1 > 0, pre1, zero)
    hq = h.float().bfloat16().to(dtype) if lowp else h
    z2 = hq @ W.t() + b2
    m = torch.where(z2 > 0, z2, zero)
    out = torch.zeros(N, H2, dtype=dtype).index_add(0, c, m)
    dm = torch.where(z2 > 0, gout[c], zero)
    dW2 = torch.zeros(H2, H1, dtype=dtype)
    dW2[:, cp] = dm.t() @ hq
    d = torch.where(pre1 > 0, dm @ W, zero)
    dpre = torch.zeros(g.nrows, H1p, dtype=dtype)
    dpre[row.unsqueeze(1), cp.unsqueeze(0)] = d
    dP, dQ = torch.zeros(N, H1p, dtype=dtype), torch.zeros(N, H1p, dtype=dtype)
    dP[:, cp] = torch.zeros(N, H1, dtype=dtype).index_add(0, c, d)
    dQ[:, cp] = torch.zeros(N, H1, dtype=dtype).index_add(0, s, d)
    r = SimpleNamespace(out=out, coords=out[:, list(coord_cols)].clone(), dW2=dW2, db2=dm.sum(0), dpre=dpre, dP=dP, dQ=dQ,
                        open1=float((pre1 > 0).double().mean()), open2=float((z2 > 0).double().mean()),
                        zeros1=int((pre1 == 0).sum()), zeros2=int((z2 == 0).sum()), coord_cols=list(coord_cols))
    if col_perm is None and edge_perm is None:
        r.row, r.c, r.s, r.m, r.d = row, c, s, m, d
    return r


def _bf(t):
    """RNE to bf16 of an fp32 value (the kernels' accumulators are fp32; on lattice inputs double -> fp32 is exact)."""
    return t.float().bfloat16().double()


def mirror_bf16(g, ref, H1p, table, ovf):
    """``out, coords, dpre, dP, dQ`` of the bf16 kernels for LATTICE inputs, from the float64 :func:`reference` ``ref``:
    the same sums, rounded to bf16 (RNE, once from the exact fp32 value) where the kernels round.  dW2 and db2 have no
    rounding point: bf16 operands that are exact, fp32 accumulation.

    ``table``: which family computes the table rows, ``"tiled"`` (edgeconv.hip) or ``"persistent"`` (edgeconv_v2.hip);
    ``ovf``: which kernels take the overflow rows, ``"tiled"`` (the OVF instances of the tiled kernels, also beside the
    persistent kernels with GN_OVF_GEMM=0) or ``"gemm"`` (``launch_ovf_*``, edgeconv.hip, the default beside the persistent
    kernels).  ``EdgePlan::persistent`` / ``EdgePlan::ovf == 2`` say which (``ops.edgeconv_plan``).  Where they differ:

    ===========  ========================================================  ==============================================
    tensor       table rows                                                overflow row of a centre (at most one)
    ===========  ========================================================  ==============================================
    ``out``      RNE(fp32 slot sum): edgeconv.hip:198, edgeconv_v2.hip     second rounding RNE(out + m): tiled adds the fp32
                 :334 and GN_WS_STORE :658 - the same in both families     message (edgeconv.hip:182), gemm adds the message
                                                                           it kept as bf16 in ``saved`` (off_ovf_m; :735)
    ``coords``   the fp32 slot sum (edgeconv.hip:199, edgeconv_v2.hip      fp32 add of the same message: unrounded (tiled,
                 :662): exact                                              :183) or the bf16 one (gemm, :736) - NOT exact
    ``dpre``     RNE(fp32 value), once: edgeconv.hip:342,                  tiled: edgeconv.hip:342; gemm: the bf16 output
                 edgeconv_v2.hip:1335 (epi_group)                          rows of the gated GEMM (launch_ovf_bwd)
    ``dP``       tiled: RNE(fp32 sum of the UNROUNDED slot values),        RNE(dP + row): tiled adds the unrounded fp32 value
                 edgeconv.hip:363-366; persistent: RNE(fp32 sum of the     (edgeconv.hip:354), gemm the bf16 dpre row
                 bf16 dpre values it staged), edgeconv_v2.hip:1362-1378    (ovf_scatter_dp_kernel, edgeconv.hip:775)
    ``dQ``       RNE(fp32 sum of the bf16 dpre rows that gathered from the source): edgeconv.hip:628-631 (one wave), :677
                 (hub kernel: fp32 partial sums); the compact gather sums the same bf16 values
    ===========  ========================================================  ==============================================
    """
    assert table in ("tiled", "persistent") and ovf in ("tiled", "gemm")
    N, H1 = g.N, int(ref.d.shape[1])
    c, s, m, d = ref.c, ref.s, ref.m, ref.d
    is_ovf = ref.row >= N * g.S
    tab = ~is_ovf
    c_o = c[is_ovf]
    cc = ref.coord_cols
    # forward
    sum_tab = torch.zeros_like(ref.out).index_add(0, c[tab], m[tab])
    m_o = _bf(m[is_ovf]) if ovf == "gemm" else m[is_ovf]
    out = _bf(sum_tab)
    out[c_o] = _bf(out[c_o] + m_o)
    coords = sum_tab[:, cc].clone()
    coords[c_o] += m_o[:, cc]
    # backward
    d_r = _bf(d)
    dP_ = _bf(torch.zeros(N, H1, dtype=torch.float64).index_add(0, c[tab], (d_r if table == "persistent" else d)[tab]))
    dP_[c_o] = _bf(dP_[c_o] + (d_r if ovf == "gemm" else d)[is_ovf])
    dQ_ = _bf(torch.zeros(N, H1, dtype=torch.float64).index_add(0, s, d_r))
    dP, dQ = torch.zeros(N, H1p, dtype=torch.float64), torch.zeros(N, H1p, dtype=torch.float64)
    dP[:, :H1], dQ[:, :H1] = dP_, dQ_
    return SimpleNamespace(out=out, coords=coords, dpre=_bf(ref.dpre), dP=dP, dQ=dQ)


def lattice_conditions(ref):
    """Why a lattice case cannot pass vacuously: about half of the gates of each layer are open, exact zeros occur at both
    (the strict ``>``), and dW2 stays inside fp32's 24 bits in units of 1/32.  Returns the list of violated conditions."""
    bad = []
    if not 0.3 <= ref.open1 <= 0.7:
        bad.append(f"open first-layer gates {ref.open1:.3f}")
    if not 0.3 <= ref.open2 <= 0.7:
        bad.append(f"open second-layer gates {ref.open2:.3f}")
    if ref.zeros1 < 1 or ref.zeros2 < 1:
        bad.append(f"exact zeros P+Q {ref.zeros1}, z2 {ref.zeros2}")
    if not float(ref.dW2.abs().max()) * 32 < 2 ** 24:
        bad.append(f"max|dW2| {float(ref.dW2.abs().max())}")
    return bad
