"""CPU: the six kernel families of the biased attention (``gn_rel_attention*``) answer their host-side questions and reject bad
arguments before any launch (there is no GPU here); ``ops._REL_FAMILY`` describes all of them and ``ops.rel_attention_family``
chooses among them."""
import pytest
import torch

from graphnet_amd import _lib, ops

FAMILIES = sorted(ops._REL_FAMILY)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


@pytest.mark.parametrize("stem", FAMILIES)
def test_supported_widths(lib, stem):
    built = ops._REL_FAMILY[stem].built
    supported = getattr(lib, f"gn_{stem}_supported")
    assert built in (32, 64)
    assert supported(built) == 1 and supported(96 - built) == 0 and supported(16) == 0
    assert getattr(ops, f"{stem}_supported")(built) is True and getattr(ops, f"{stem}_supported")(96 - built) is False


@pytest.mark.parametrize("fault", ["head width", "null pointer", "pitch"])
@pytest.mark.parametrize("stem", FAMILIES)
def test_bad_arguments_are_rejected_on_the_host(lib, stem, fault):
    fam = ops._REL_FAMILY[stem]
    H, B, N = 2, 1, 8
    DH = 96 - fam.built if fault == "head width" else fam.built
    d = H * DH
    p = None if fault == "null pointer" else 256           # (never dereferenced: every fault returns before the launch)
    off = 2 if fam.rows == torch.float32 else 4            # a row pitch that is no multiple of 4 floats / 8 bf16
    ld = 3 * d + off if fault == "pitch" else 3 * d
    rc = getattr(lib, f"gn_{stem}_fwd")(p, ld, p, d, p, 4, p, H, DH, p, p, B, N, p, d, p, d, p, None)
    err = lib.gn_last_error()
    assert rc != 0 and f"gn_{stem}_fwd:".encode() in err and fault.encode() in err
    if fault != "null pointer":
        assert f"head width {fam.built},".encode() in err
    rc = getattr(lib, f"gn_{stem}_bwd")(p, ld, p, d, p, 4, p, H, DH, p, p, B, N, p, d, p, d, p, d, p, d, p, p, p, 3 * d, p, d, None)
    err = lib.gn_last_error()
    assert rc != 0 and f"gn_{stem}_bwd:".encode() in err and fault.encode() in err


@pytest.mark.parametrize("stem", FAMILIES)
def test_an_empty_batch_returns_before_any_launch(lib, stem):
    H, DH, B, p = 2, ops._REL_FAMILY[stem].built, 1, None
    d = H * DH
    assert getattr(lib, f"gn_{stem}_fwd")(p, 3 * d, p, d, p, 4, p, H, DH, p, p, B, 0, p, d, p, d, p, None) == 0
    assert getattr(lib, f"gn_{stem}_bwd")(p, 3 * d, p, d, p, 4, p, H, DH, p, p, B, 0, p, d, p, d, p, d, p, d, p, p, p, 3 * d, p, d,
                                          None) == 0


def test_family_selection_truth_table():
    table = {(32, False, False): "rel_attention", (32, True, False): "rel_attention_shared",
             (32, False, True): "rel_attention_mfma", (32, True, True): "rel_attention_mfma",
             (64, False, False): "rel_attention_wide", (64, True, False): "rel_attention_wide_shared",
             (64, False, True): "rel_attention_mfma_wide", (64, True, True): "rel_attention_mfma_wide"}
    for (dh, shared, matrix), stem in table.items():
        assert ops.rel_attention_family(dh, shared=shared, matrix=matrix) == stem
    assert ops.rel_attention_family(32) == "rel_attention" and ops.rel_attention_family(64) == "rel_attention_wide"
    assert set(table.values()) == set(ops._REL_FAMILY)
    for dh in (8, 16, 48, 128):
        for shared in (False, True):
            for matrix in (False, True):
                assert ops.rel_attention_family(dh, shared=shared, matrix=matrix) is None


def test_the_table_is_complete(lib):
    assert len(ops._REL_FAMILY) == 6
    for stem in ops._REL_FAMILY:
        for which in ("supported", "fwd", "bwd"):
            assert hasattr(lib, f"gn_{stem}_{which}")
            fn = getattr(ops, f"{stem}_{which}")
            assert callable(fn) and fn.__name__ == f"{stem}_{which}" and fn.__doc__
    assert ops.rel_attention_run_fwd.__doc__ and ops.rel_attention_run_bwd.__doc__
    for which in ("fwd", "bwd"):
        argtypes = [list(getattr(lib, f"gn_{stem}_{which}").argtypes) for stem in FAMILIES]
        assert argtypes[0] and all(a == argtypes[0] for a in argtypes)
