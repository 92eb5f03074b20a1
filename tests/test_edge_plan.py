"""CPU: which kernels a fused EdgeConv layer runs is decided in one place (graphnet_amd/csrc/edge_plan.hpp).

(a) pins what the host-only query entries of the built library answer (no GPU: the CU count falls back to 256; every
    tile count below stays under 125, so the values hold for any device with 250 CUs or more);
(b) compiles edge_plan.hpp alone with the host C++ compiler and compares edge_plan() with a table derived by hand from
    the dispatch rules, once more under AddressSanitizer + UBSan (a stand-alone binary)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphnet_amd", "csrc")


@pytest.fixture(scope="module")
def lib_path():
    from graphnet_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.LIB_PATH


@pytest.fixture(scope="module")
def lib(lib_path):
    return ctypes.CDLL(lib_path)          # int arguments, int results: the ctypes defaults


# ---------------------------------------------------------------------------------------------- (a) query entries
def test_dw2_slab_counts(lib):
    # 1000 nodes x 8 slots = 125 tiles of 64 rows: 125 tile parts (H1p = 352: min(256 / 2 halves, 125)) + 128 overflow splits
    assert lib.gn_edgeconv_dw2_slabs(1, 1000, 8, 352, 256) == 253
    assert lib.gn_edgeconv_dw2_slabs(1, 1000, 8, 128, 256) == 253
    # outside the persistent envelope: ceil((N * S + N) / 4096) row ranges of the tiled kernel
    assert lib.gn_edgeconv_dw2_slabs(1, 1000, 8, 256, 256) == 3
    assert lib.gn_edgeconv_dw2_slabs(0, 1000, 8, 352, 256) == 3
    assert lib.gn_edgeconv_dw2_slabs(1, 1000, 17, 352, 256) == 9          # 32 slots: ceil(33000 / 4096)
    assert lib.gn_edgeconv_max_dw2_slabs(1000, 8, 256) == 125


def test_disable_v2_is_read_on_every_call(lib):
    old = os.environ.get("GN_DISABLE_V2")
    try:
        os.environ["GN_DISABLE_V2"] = "1"
        assert lib.gn_edgeconv_dw2_slabs(1, 1000, 8, 352, 256) == 3
        assert lib.gn_edgeconv_leaky_supported(1, 8, 352, 336, 256) == 0
        assert lib.gn_edgeconv_max_supported(1, 16, 256, 256) == 0
    finally:
        if old is None:
            os.environ.pop("GN_DISABLE_V2", None)
        else:
            os.environ["GN_DISABLE_V2"] = old
    assert lib.gn_edgeconv_dw2_slabs(1, 1000, 8, 352, 256) == 253


def test_supported_queries(lib):
    assert lib.gn_edgeconv_leaky_supported(1, 8, 352, 336, 256) == 1
    assert lib.gn_edgeconv_leaky_supported(1, 8, 352, 340, 256) == 0
    assert lib.gn_edgeconv_leaky_supported(1, 8, 128, 128, 256) == 1
    assert lib.gn_edgeconv_leaky_supported(0, 8, 352, 336, 256) == 0
    assert lib.gn_edgeconv_max_supported(1, 16, 256, 256) == 1
    assert lib.gn_edgeconv_max_supported(1, 8, 352, 256) == 0
    assert lib.gn_edgeconv_max_supported(1, 17, 256, 256) == 0
    assert lib.gn_edgeconv_max_supported(0, 16, 256, 256) == 0


def test_compact_dpre_is_opt_in(lib_path):
    env = {k: v for k, v in os.environ.items() if k != "GN_DPRE_COMPACT"}
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); f = l.gn_edgeconv_dpre_compact_supported; "
            "print(f(1, 8, 352, 336, 256), f(1, 8, 352, 348, 256))")
    # the switch is read once per process: a fresh child each
    off = subprocess.run([sys.executable, "-c", code, lib_path], env=env, stdout=subprocess.PIPE, text=True, check=True)
    assert off.stdout.split() == ["0", "0"]
    env["GN_DPRE_COMPACT"] = "1"
    on = subprocess.run([sys.executable, "-c", code, lib_path], env=env, stdout=subprocess.PIPE, text=True, check=True)
    assert on.stdout.split() == ["1", "0"]                    # H1 = 348: 44 chunks > 43


# ------------------------------------------------------------------------------------------------- (b) plan table
MAIN = r"""
#include "edge_plan.hpp"
#include <cstdio>
// stdin: mode K N H1p H1 H2 act has_ovf disable_v2 ovf_gemm dpre_compact per line -> the plan's fields
int main() {
    int mode, K, H1p, H1, H2, act, ovf, dis, og, dc;
    long long N;
    while (std::scanf("%d %d %lld %d %d %d %d %d %d %d %d", &mode, &K, &N, &H1p, &H1, &H2, &act, &ovf, &dis, &og, &dc) == 11) {
        gn::EdgeSwitches sw = {};
        sw.disable_v2 = dis != 0; sw.ovf_gemm = og != 0; sw.dpre_compact = dc != 0; sw.edge_ws = 7; sw.producers_first = 0;
        const gn::EdgePlan p = gn::edge_plan(mode, K, N, H1p, H1, H2, act, ovf != 0, sw);
        std::printf("%d %d %d %d %d %d %d\n", (int)p.supported, (int)p.persistent, p.variant, p.ovf, (int)p.compact_shape,
                    (int)p.compact_model, (int)p.shape_persistent);
    }
    return 0;
}
"""

DEF = (0, 1, 0)          # switches: disable_v2, ovf_gemm, dpre_compact
TILED, PERS = 0, 1
# ((mode, K, N, H1p, H1, H2, act, has_ovf), switches) -> (supported, persistent, variant, ovf, compact_shape, compact_model,
# shape_persistent)
CASES = [
    (((1, 8, 1000, 352, 336, 256, 0, 1), DEF), (1, PERS, 0, 2, 1, 0, 1)),
    (((1, 8, 1000, 352, 340, 256, 0, 1), DEF), (1, PERS, 0, 2, 1, 0, 1)),           # relu: the real width does not decide
    (((1, 16, 1000, 128, 128, 256, 0, 1), DEF), (1, PERS, 0, 2, 1, 0, 1)),
    (((1, 8, 1000, 352, 336, 256, 0, 0), DEF), (1, PERS, 0, 0, 1, 0, 1)),
    (((1, 17, 1000, 352, 336, 256, 0, 1), DEF), (1, TILED, 0, 1, 0, 0, 0)),         # 32 slots
    (((1, 8, 1000, 256, 256, 256, 0, 1), DEF), (1, TILED, 0, 1, 0, 0, 0)),          # hidden width outside the envelope
    (((1, 8, 1000, 352, 336, 128, 0, 1), DEF), (1, TILED, 0, 1, 0, 0, 0)),          # output width
    (((0, 8, 1000, 352, 336, 256, 0, 1), DEF), (1, TILED, 0, 1, 0, 0, 0)),          # fp32
    (((1, 8, 3_100_000, 352, 336, 256, 0, 1), DEF), (1, PERS, 0, 1, 1, 0, 1)),      # N * H1p * 2 >= 2^31: no GEMM overflow path
    (((1, 8, 1000, 352, 336, 256, 2, 1), DEF), (1, PERS, 2, 2, 0, 0, 1)),
    # leaky + add needs H1 <= 336: tiled kernels for table AND overflow rows (never the GEMM path next to the tiled family);
    # the dW2 slabs are still counted as for the shape
    (((1, 8, 1000, 352, 340, 256, 2, 1), DEF), (1, TILED, 2, 1, 0, 0, 1)),
    (((1, 8, 1000, 128, 100, 256, 2, 0), DEF), (1, PERS, 2, 0, 0, 0, 1)),
    (((1, 16, 1000, 256, 256, 256, 1, 0), DEF), (1, PERS, 1, 0, 0, 0, 1)),
    (((1, 16, 1000, 256, 256, 256, 1, 1), DEF), (0, TILED, 1, 0, 0, 0, 1)),         # leaky + max: no overflow rows ...
    (((1, 8, 1000, 352, 336, 256, 1, 0), DEF), (0, TILED, 1, 0, 0, 0, 0)),          # ... (256, 256) only ...
    (((0, 16, 1000, 256, 256, 256, 1, 0), DEF), (0, TILED, 1, 0, 0, 0, 0)),         # ... bf16 only
    (((1, 8, 1000, 352, 336, 256, 3, 0), DEF), (0, TILED, 3, 0, 0, 0, 0)),          # no such variant
    # other switches
    (((1, 8, 1000, 352, 336, 256, 0, 1), (1, 1, 0)), (1, TILED, 0, 1, 0, 0, 0)),
    (((1, 16, 1000, 256, 256, 256, 1, 0), (1, 1, 0)), (0, TILED, 1, 0, 0, 0, 0)),
    (((1, 8, 1000, 352, 336, 256, 0, 1), (0, 0, 0)), (1, PERS, 0, 1, 1, 0, 1)),
    (((1, 8, 1000, 352, 336, 256, 0, 1), (0, 1, 1)), (1, PERS, 0, 2, 1, 1, 1)),
    (((1, 8, 1000, 128, 128, 256, 0, 1), (0, 1, 1)), (1, PERS, 0, 2, 1, 1, 1)),
    (((1, 8, 1000, 352, 348, 256, 0, 1), (0, 1, 1)), (1, PERS, 0, 2, 0, 0, 1)),     # 44 chunks > 43
    (((1, 8, 1000, 352, 336, 256, 2, 1), (0, 1, 1)), (1, PERS, 2, 2, 0, 0, 1)),
    (((1, 8, 1000, 352, 336, 256, 0, 1), (1, 1, 1)), (1, TILED, 0, 1, 0, 0, 0)),
]


def _plan_table(tmp_path, flags):
    (tmp_path / "plan_main.cpp").write_text(MAIN)
    exe = tmp_path / ("plan" + "_san" * bool(flags))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, str(tmp_path / "plan_main.cpp"), "-o", str(exe)],
                   check=True)
    text = "".join(" ".join(str(v) for v in args + sw) + "\n" for (args, sw), _ in CASES)
    out = subprocess.run([str(exe)], input=text, stdout=subprocess.PIPE, text=True, check=True).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def test_plan_query_entry_answers_with_the_plan(lib_path):
    """gn_edgeconv_plan (what the GPU tests name their path by) = the same table, under the switches of ITS process: a
    fresh child per switch set (read once per process); the eighth field says whether the persistent forward is the
    wave-specialised kernel (relu: GN_EDGE_WS bit 0, and H1 <= 336 or H1p = 128)."""
    code = ("import ctypes, sys; l = ctypes.CDLL(sys.argv[1]); o = (ctypes.c_int32 * 8)()\n"
            "for line in sys.stdin:\n"
            "    a = [int(v) for v in line.split()]\n"
            "    l.gn_edgeconv_plan(a[0], a[1], ctypes.c_int64(a[2]), *a[3:8], o); print(*o)\n")
    switches = ("GN_DISABLE_V2", "GN_OVF_GEMM", "GN_DPRE_COMPACT", "GN_EDGE_WS")
    for sw in sorted({sw for (_, sw), _ in CASES}):
        rows = [(args, want) for (args, s), want in CASES if s == sw]
        for edge_ws in (None, "0"):
            env = {k: v for k, v in os.environ.items() if k not in switches}
            env.update(GN_DISABLE_V2=str(sw[0]), GN_OVF_GEMM=str(sw[1]), GN_DPRE_COMPACT=str(sw[2]))
            if edge_ws is not None:
                env["GN_EDGE_WS"] = edge_ws
            text = "".join(" ".join(str(v) for v in args) + "\n" for args, _ in rows)
            out = subprocess.run([sys.executable, "-c", code, lib_path], env=env, input=text, stdout=subprocess.PIPE, text=True,
                                 check=True).stdout
            got = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
            assert len(got) == len(rows)
            for (args, want), have in zip(rows, got):
                _, _, N, H1p, H1, _, act, _ = args
                ws = want[1] == PERS and (act != 0 or (edge_ws is None and (H1p == 128 or H1 <= 336)))
                ws = ws and N * 4 * H1p < 2 ** 32                 # the wave-specialised kernel's 32-bit P|Q byte offsets
                assert have == want + (int(ws),), (args, sw, edge_ws, have, want)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_plan_table(tmp_path, flags):
    got = _plan_table(tmp_path, flags)
    assert len(got) == len(CASES)
    for ((args, sw), want), have in zip(CASES, got):
        assert have == want, (args, sw, have, want)
