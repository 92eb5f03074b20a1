"""Every kernel path of the fused ReLU edge convolution (``gn_edgeconv_fwd``, ``gn_edgeconv_dw2`` + ``_dw2_reduce``,
``gn_edgeconv_bwd``, ``gn_edgeconv_dq_gather`` and the compact-dpre pair) against the float64 reference of
``tests/edgeconv_reference.py`` - every output of the three passes, ``dpre`` included, ``dP`` and ``dQ`` apart.

Paths (``ops.edgeconv_plan`` - the dispatch rule's own answer - names the one that runs and skips a shape outside it):

    fp32                        mode 0: the tiled kernels
    bf16_tiled                  mode 1 with GN_DISABLE_V2=1
    bf16_persistent             mode 1: persistent kernels, overflow rows on the GEMM kernels
    bf16_compact                ... with ``ops.edgeconv_bwd_gather_compact`` for dP | dQ
    bf16_persistent_ovf_tiled   GN_OVF_GEMM=0: persistent kernels beside the tiled overflow-row kernels   } read once per
    bf16_fwd_no_ws              GN_EDGE_WS=0: the persistent forward without wave specialisation          } process: a child

Shapes (k, H1, H2): (8, 336, 256) and (8, 128, 256) the two persistent envelopes; (16, 336, 256) 16 slots, uint16 slot
masks; (12, 128, 256) 16 slots with empty columns; (8, 340, 256) real columns in the last k-step, compact still allowed;
(8, 348, 256) above the compact limit; (5, 100, 96) tiled kernels only, H2 != 256, H1 no multiple of 32; and (8, 336, 256)
on a strict table (no overflow list).  One batch for all: events of 1, 3, 2, 9, 70 and 110 pulses with crafted ties
(``edgeconv_reference.batch_coords``); its features are asserted, not assumed.

Every output buffer the caller owns (``out``, ``dpre``, both halves of ``dPQ`` with their pad columns) is filled with NaN
first, as the model hands the kernels ``torch.empty`` memory: an element a kernel fails to write fails the comparison.
Only the ``dpre`` rows at and beyond N * S + cnt may stay NaN, and nothing may read them.

LATTICE inputs (exact in bf16 and fp32, every partial sum exact in fp32): bit-for-bit equalities.

    fp32:  out, coords, dW2, db2, dpre, dP, dQ == the float64 reference
    bf16:  dW2, db2 == the float64 reference (exact operands, fp32 accumulation);
           out, coords, dpre, dP, dQ == ``mirror_bf16`` (the reference with the path's bf16 roundings, each cited there);
           coords == the float64 reference as well wherever no rounded value enters it: every centre on the tiled
           overflow kernels, the centres without an overflow row on the GEMM path (which adds the bf16 message)
    bf16_compact: dP | dQ == bf16_persistent == the mirror

(The sign of an exact zero depends on the summation order - (+0) + (-0) = +0 - so -0.0 and +0.0 compare equal.)

REAL-VALUED inputs (the generator of ``test_gpu_leaky.py``): the project's gates - out 1e-4 (fp32) / 2e-2 (bf16) of the
tensor's max, dW2, db2, dP, dQ and dpre Frobenius 5e-3 / 2e-2 - with the measured errors appended to the parity report
that ``tests/test_gpu_model.py::_parity_report`` keeps."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import edgeconv_reference as er
from test_gpu_model import _parity_report          # the one record of how far inside its gate each tensor sits

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
IN_PROCESS = ["fp32", "bf16_tiled", "bf16_persistent", "bf16_compact"]
CHILD = {"bf16_persistent_ovf_tiled": ("GN_OVF_GEMM", "0"), "bf16_fwd_no_ws": ("GN_EDGE_WS", "0")}
LATTICE_KEYS = ("out", "coords", "dW2", "db2", "dpre", "dP", "dQ")


# ---------------------------------------------------------------------------------------------------- case and run
@functools.lru_cache(maxsize=None)
def _case(case):
    """Device table, its host copy and, per input kind and operand type, inputs + float64 reference: built once per
    (k, H1, H2, strict) and shared by every path (nothing here is modified afterwards)."""
    from graphnet_amd import ops
    k, H1, H2, strict = case
    x, ptr = er.batch_coords(k)
    ptr32 = ptr.to(torch.int32).to(DEV)
    batch32 = torch.repeat_interleave(torch.arange(len(er.SIZES), dtype=torch.int32), torch.tensor(er.SIZES)).to(DEV)
    g = ops.knn_graph(x.to(DEV), [0, 1, 2], batch32, ptr32, k, strict=strict)
    hg = er.HostGraph.from_table(g)
    g.build_reverse()
    f = hg.features()
    assert (g.ovf is None and f["ovf_cnt"] == 0) if strict else f["ovf_cnt"] > 0, f
    assert f["max_in_degree"] > 64 and int(g.rev_nhubs[0]) > 0, f
    assert f["centres_without_edge"] >= 1 and f["sources_without_in_edge"] >= 1 and f["empty_slots"] >= 1, f
    assert f["n_mod_8"] != 0 and f["partial_last_tile"] and hg.S == g.S, f
    return dict(g=g, hg=hg, H1p=er.round_up(H1, 32))


@functools.lru_cache(maxsize=None)
def _inputs(case, kind, lowp):
    k, H1, H2, _ = case
    c = _case(case)
    hg, H1p = c["hg"], c["H1p"]
    adt = torch.bfloat16 if lowp else torch.float32
    if kind == "lattice":
        PQ, W2, b2, gout = er.lattice_inputs(hg.N, H1, H1p, H2)
        PQ, gout = PQ.to(adt), gout.to(adt)                           # exact in either type
    else:
        PQ, W2, b2, gout = er.real_inputs(hg.N, k, H1, H1p, H2, adt)
    ref = er.reference(hg, PQ, H1p, H1, W2, b2, gout, lowp=lowp and kind == "real")
    if kind == "lattice":
        assert er.lattice_conditions(ref) == [], er.lattice_conditions(ref)
    return dict(PQ=PQ, W2=W2, b2=b2, gout=gout, ref=ref)


def _run(case, kind, mode, compact=False, forward_only=False):
    """The passes of one layer on poisoned output buffers -> CPU tensors."""
    from graphnet_amd import ops
    _, H1, H2, _ = case
    c, i = _case(case), _inputs(case, kind, mode == 1)
    g, H1p, N = c["g"], c["H1p"], c["hg"].N
    dt, adt = ops.mode_dtype(mode), ops.act_dtype(mode)
    PQ, W2, b2, gout = i["PQ"].to(DEV), i["W2"].to(DEV), i["b2"].to(DEV), i["gout"].to(DEV)
    W2p, W2Tp = ops.pack_weight(W2, [H1], dt), ops.pack_weight(W2.t().contiguous(), [H2], dt)
    out = torch.full((N, H2), NAN, dtype=adt, device=DEV)
    out, saved, coords = ops.edgeconv_fwd(mode, g, PQ, H1p, W2p, b2, H2, out=out, coord_cols=list(er.COORD_COLS), H1=H1)
    res = dict(out=out, coords=coords[:, :len(er.COORD_COLS)])
    if not forward_only:
        res["dW2"], res["db2"] = ops.edgeconv_dw2(mode, g, PQ, H1p, H1, H2, gout, saved)     # slabs: torch.empty, as always
        dPQ = torch.full((N, 2 * H1p), NAN, dtype=adt, device=DEV)
        if compact:
            ops.edgeconv_bwd_gather_compact(g, PQ, H1p, H1, H2, gout, saved, W2Tp, dPQ)
        else:
            dpre = torch.full((max(g.rows, 1), H1p), NAN, dtype=dt, device=DEV)
            ops.edgeconv_bwd(mode, g, PQ, H1p, H2, gout, saved, W2Tp, dpre, dPQ[:, :H1p])
            ops.edgeconv_dq_gather(mode, g, dpre, H1p, dPQ[:, H1p:])
            res["dpre"] = dpre
        res["dP"], res["dQ"] = dPQ[:, :H1p], dPQ[:, H1p:]
    torch.cuda.synchronize()
    return {k_: v.detach().cpu() for k_, v in res.items()}


# ------------------------------------------------------------------------------------------------------ comparisons
def _same(a, b):
    """Bit-for-bit equality of ``a`` with the float64 expectation ``b`` in a's type (+0.0 == -0.0; a NaN equals nothing)."""
    b64, b = b, b.to(a.dtype)
    assert torch.equal(b.double(), b64.double()) and a.shape == b.shape     # the expectation is a number of a's type
    bad = ~(a == b)
    if not bool(bad.any()):
        return None
    idx = torch.nonzero(bad)
    first = tuple(int(v) for v in idx[0])
    return dict(mismatches=int(bad.sum()), of=a.numel(), nan=int(torch.isnan(a).sum()), first=list(first),
                got=float(a[first]), want=float(b[first]), rows=int(idx[:, 0].unique().numel()))


def _check_lattice(case, got, plan, keys):
    """-> {key: None | mismatch record}; an empty record list means every equality of the module docstring holds."""
    _, H1, _, _ = case
    c = _case(case)
    hg, H1p = c["hg"], c["H1p"]
    fp32 = got["out"].dtype == torch.float32
    ref = _inputs(case, "lattice", not fp32)["ref"]
    want = {k: getattr(ref, k) for k in LATTICE_KEYS}
    if not fp32:
        mir = er.mirror_bf16(hg, ref, H1p, "persistent" if plan["persistent"] else "tiled", "gemm" if plan["ovf"] == 2 else "tiled")
        want.update(out=mir.out, coords=mir.coords, dpre=mir.dpre, dP=mir.dP, dQ=mir.dQ)
    bad = {}
    for k in keys:
        a = got[k][:hg.nrows] if k == "dpre" else got[k]               # rows >= N * S + cnt: nobody's, may stay NaN
        r = _same(a, want[k])
        if r is not None:
            bad[k] = r
    if not fp32 and "coords" in keys:                                 # exact wherever no bf16 message entered
        plain = torch.ones(hg.N, dtype=torch.bool)
        if plan["ovf"] == 2:
            plain[hg.ovf_centre] = False
        r = _same(got["coords"][plain], ref.coords[plain])
        if r is not None:
            bad["coords_vs_float64"] = r
    for k in ("dpre", "dP", "dQ"):                                    # pad columns: written, and exactly 0
        if k in keys and H1 < H1p:
            a = got[k][:hg.nrows] if k == "dpre" else got[k]
            if not bool((a[:, H1:] == 0).all()):
                bad[k + "_pad"] = dict(nonzero=int((a[:, H1:] != 0).sum()), nan=int(torch.isnan(a[:, H1:]).sum()))
    for k in keys:                                                    # nothing read the rows that stayed NaN
        a = got[k][:hg.nrows] if k == "dpre" else got[k]
        if not bool(torch.isfinite(a).all()):
            bad[k + "_finite"] = int((~torch.isfinite(a)).sum())
    return bad


def _norm_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _check_real(case, got, keys):
    """-> (errors, gates): the project's gates of test_gpu_leaky.py, dP and dQ apart, dpre at the gradients' gate."""
    hg = _case(case)["hg"]
    fp32 = got["out"].dtype == torch.float32
    ref = _inputs(case, "real", not fp32)["ref"]
    errs, gates = {}, {}
    for k in keys:
        a = got[k][:hg.nrows] if k == "dpre" else got[k]
        if k in ("out", "coords"):
            errs[k], gates[k] = _rel_err(a, getattr(ref, k)), (1e-4 if fp32 else 2e-2)
        else:
            errs[k], gates[k] = _norm_err(a, getattr(ref, k)), (5e-3 if fp32 else 2e-2)
        if not bool(torch.isfinite(a).all()):
            errs[k] = float("inf")
    return errs, gates


def _plan(case, mode):
    from graphnet_amd import ops
    _, H1, H2, _ = case
    c = _case(case)
    return ops.edgeconv_plan(mode, c["g"], c["H1p"], H1, H2)


def _one_case(path, case):
    """Lattice + real-valued run of ``case`` on ``path`` -> JSON-able record (``skipped``: outside the path's envelope)."""
    mode = 0 if path == "fp32" else 1
    compact, forward_only = path == "bf16_compact", path == "bf16_fwd_no_ws"
    rec = dict(path=path, case=er.case_id(case))
    old = os.environ.get("GN_DISABLE_V2")
    if path == "bf16_tiled":
        os.environ["GN_DISABLE_V2"] = "1"
    try:
        plan = _plan(case, mode)
        rec["plan"] = plan
        assert plan["supported"]
        has_ovf = _case(case)["hg"].cnt > 0
        # the path this parameter means to test is the one the dispatch takes - or the shape is outside its envelope
        if path in ("fp32", "bf16_tiled"):
            assert not plan["persistent"] and plan["ovf"] == (1 if has_ovf else 0), plan
        elif not plan["persistent"] or (compact and not plan["compact_shape"]):
            rec["skipped"] = "outside the envelope of the persistent kernels" if not plan["persistent"] else \
                "outside the envelope of the compact-dpre kernels"
            return rec
        elif path == "bf16_persistent_ovf_tiled":
            assert plan["ovf"] == (1 if has_ovf else 0), plan
        elif path == "bf16_fwd_no_ws":
            assert not plan["fwd_ws"], plan
        else:
            assert plan["ovf"] == (2 if has_ovf else 0), plan
        keys = [k for k in LATTICE_KEYS if not (forward_only and k not in ("out", "coords")) and not (compact and k == "dpre")]
        got = _run(case, "lattice", mode, compact, forward_only)
        rec["lattice_bad"] = _check_lattice(case, got, plan, keys)
        if compact:                                                   # ... and bit-identical to the dense pair, as before
            dense = _run(case, "lattice", mode)
            rec["compact_equals_dense"] = all(torch.equal(got[k].view(torch.int16), dense[k].view(torch.int16)) for k in ("dP", "dQ"))
        got = _run(case, "real", mode, compact, forward_only)
        rec["real_err"], rec["real_gate"] = _check_real(case, got, keys)
    finally:
        if path == "bf16_tiled":
            if old is None:
                os.environ.pop("GN_DISABLE_V2", None)
            else:
                os.environ["GN_DISABLE_V2"] = old
    return rec


def _assert_record(rec):
    if "skipped" in rec:
        return
    assert rec["lattice_bad"] == {}, (rec["path"], rec["case"], rec["lattice_bad"])
    assert rec.get("compact_equals_dense", True), (rec["path"], rec["case"])
    _parity_report(f"edgeconv_relu[{rec['path']}-{rec['case']}]", rec["real_err"])
    for k, e in rec["real_err"].items():
        assert e < rec["real_gate"][k], (rec["path"], rec["case"], k, e, rec["real_gate"][k])


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("case", er.CASES, ids=er.case_id)
@pytest.mark.parametrize("path", IN_PROCESS)
def test_relu_edgeconv_against_float64(path, case):
    rec = _one_case(path, case)
    if "skipped" in rec:
        pytest.skip(f"{path} {rec['case']}: {rec['skipped']} (plan {rec['plan']})")
    _assert_record(rec)


def child_main(path):
    """Body of the child process of a path whose switch is read once per process: every case, one JSON line each."""
    var, val = CHILD[path]
    assert os.environ.get(var) == val
    for case in er.CASES:
        print("EDGECONV_CASE " + json.dumps(_one_case(path, case)), flush=True)


@pytest.mark.parametrize("path", list(CHILD))
def test_relu_edgeconv_paths_behind_process_wide_switches(path):
    """GN_OVF_GEMM=0 / GN_EDGE_WS=0 select kernels no other test runs.  One fresh child per path (so at most one extra GPU
    process at a time) runs all cases and reports; a child that dies or runs out of time fails the test, no retry."""
    var, val = CHILD[path]
    # the switch must change something: in THIS process the same shapes take the other path
    assert os.environ.get(var) is None, f"{var} is set for the whole suite"
    base = _plan(er.CASES[0], 1)
    assert base["persistent"] and base["ovf"] == 2 and base["fwd_ws"], base
    env = dict(os.environ)
    env[var] = val
    env.pop("GN_DISABLE_V2", None)
    code = f"import sys; sys.path.insert(0, {TESTS!r}); sys.path.insert(0, {ROOT!r}); import test_gpu_edgeconv_relu as t; t.child_main({path!r})"
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=240)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    recs = [json.loads(line[len("EDGECONV_CASE "):]) for line in p.stdout.splitlines() if line.startswith("EDGECONV_CASE ")]
    assert [r["case"] for r in recs] == [er.case_id(c) for c in er.CASES]
    ran = [r for r in recs if "skipped" not in r]
    print(f"{path}: ran {[r['case'] for r in ran]}, skipped {[(r['case'], r['skipped']) for r in recs if 'skipped' in r]}")
    assert len(ran) >= 6                                              # every shape of the persistent envelope
    if path == "bf16_persistent_ovf_tiled":
        assert any(r["plan"]["ovf"] == 1 for r in ran)
    for r in recs:
        _assert_record(r)
