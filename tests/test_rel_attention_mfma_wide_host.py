"""CPU: the head-width-64 matrix-core entries of the biased attention (``gn_rel_attention_mfma_wide_*``) answer their host-side
questions and reject bad arguments before any launch (there is no GPU here)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from graphnet_amd import _lib
    return _lib.lib()


def test_supported_widths(lib):
    assert lib.gn_rel_attention_mfma_wide_supported(64) == 1
    assert lib.gn_rel_attention_mfma_wide_supported(32) == 0 and lib.gn_rel_attention_mfma_wide_supported(16) == 0
    assert lib.gn_rel_attention_mfma_supported(64) == 0 and lib.gn_rel_attention_mfma_supported(32) == 1


@pytest.mark.parametrize("fault", ["head width", "null pointer", "pitch"])
def test_bad_arguments_are_rejected_on_the_host(lib, fault):
    H, B, N = 2, 1, 8
    DH = 32 if fault == "head width" else 64
    d = H * DH
    p = None if fault == "null pointer" else 256           # (never dereferenced: every fault returns before the launch)
    ld = 3 * d + 4 if fault == "pitch" else 3 * d          # a row pitch that is no multiple of 8 bf16
    rc = lib.gn_rel_attention_mfma_wide_fwd(p, ld, p, d, p, 4, p, H, DH, p, p, B, N, p, d, p, d, p, None)
    assert rc != 0 and b"gn_rel_attention_mfma_wide_fwd" in lib.gn_last_error() and fault.encode() in lib.gn_last_error()
    rc = lib.gn_rel_attention_mfma_wide_bwd(p, ld, p, d, p, 4, p, H, DH, p, p, B, N, p, d, p, d, p, d, p, d, p, p, p, 3 * d, p, d, None)
    assert rc != 0 and b"gn_rel_attention_mfma_wide_bwd" in lib.gn_last_error() and fault.encode() in lib.gn_last_error()
