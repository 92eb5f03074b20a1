"""Regenerates ``ice_transparency.npz`` and ``icemix_nodes_expected.npz``: the table the REFERENCE's ``ice_transparency()``
reads (110 rows of depth, scattering length, absorption length) and what the two functions it returns give.  Only the
recorded numbers are stored.

    python tests/golden/make_icemix_fixtures.py <root of the reference>

``models/graphs/utils.py`` pulls in packages that this project does not need, so the one function definition the recipe
uses is taken out of its syntax tree at run time and executed against pandas, scipy and sklearn (needed here only).

For the default ``ice_args`` ("d_") and one non-default pair ("o_", ``z_offset = -1900``, ``z_scaling = 450``):

* ``*_z_norm``, ``*_scatt``, ``*_abs``: the knots of the two ``interp1d`` functions, fp64 (``f.x`` / ``f.y``).
* ``*_z``: fp32 evaluation points inside the table's range: the z of every IceCube-86 DOM divided by 500, every knot rounded
  to fp32 with its two fp32 neighbours, and 4000 uniform draws.
* ``*_fs64`` / ``*_fa64``: the functions at those points as returned (fp64);  ``*_fs32`` / ``*_fa32``: rounded to fp32.
"""
import ast
import os
import sys
from typing import Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CASES = {"d_": {"z_offset": None, "z_scaling": None}, "o_": {"z_offset": -1900.0, "z_scaling": 450.0}}


def reference_function(reference_root: str):
    import pandas as pd
    from scipy.interpolate import interp1d
    from sklearn.preprocessing import RobustScaler
    utils_py = os.path.join(reference_root, "src", "graphnet", "models", "graphs", "utils.py")
    tree = ast.parse(open(utils_py).read())
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "ice_transparency"]
    assert len(body) == 1
    ns = {"np": np, "pd": pd, "os": os, "Tuple": Tuple, "interp1d": interp1d, "RobustScaler": RobustScaler,
          "DATA_DIR": os.path.join(reference_root, "data")}
    exec(compile(ast.Module(body=body, type_ignores=[]), utils_py, "exec"), ns)
    return ns["ice_transparency"]


def points(z_norm: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    dom_z = np.load(os.path.join(ROOT, "graphnet_amd", "geometry_tables", "icecube86.npz"))["table"][:, 2]
    knots = z_norm.astype(np.float32)
    z = np.concatenate([
        (dom_z[np.isfinite(dom_z)].astype(np.float32) / np.float32(500.0)).astype(np.float32),
        knots, np.nextafter(knots, np.float32(-np.inf)), np.nextafter(knots, np.float32(np.inf)),
        rng.uniform(z_norm[0], z_norm[-1], 4000).astype(np.float32),
    ]).astype(np.float32)
    zd = z.astype(np.float64)
    return z[(zd >= z_norm[0]) & (zd <= z_norm[-1])]


def main() -> None:
    import pandas as pd
    root = sys.argv[1]
    ice_transparency = reference_function(root)
    df = pd.read_parquet(os.path.join(root, "data", "ice_properties", "ice_transparency.parquet"))
    table = {k: np.asarray(df[k], dtype=np.float64) for k in ("depth", "scattering_len", "absorption_len")}
    np.savez_compressed(os.path.join(HERE, "ice_transparency.npz"), **table)
    rng = np.random.default_rng(20261021)
    out = {}
    for tag, ice_args in CASES.items():
        f_s, f_a = ice_transparency(**ice_args)
        assert np.array_equal(f_s.x, f_a.x)
        z = points(f_s.x, rng)
        out[tag + "z_norm"], out[tag + "scatt"], out[tag + "abs"] = f_s.x, f_s.y, f_a.y
        out[tag + "z"] = z
        out[tag + "fs64"], out[tag + "fa64"] = np.asarray(f_s(z), np.float64), np.asarray(f_a(z), np.float64)
        out[tag + "fs32"], out[tag + "fa32"] = out[tag + "fs64"].astype(np.float32), out[tag + "fa64"].astype(np.float32)
        out[tag + "ice_args"] = np.asarray([np.nan if v is None else v for v in ice_args.values()], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "icemix_nodes_expected.npz"), **out)
    print({k: v.shape for k, v in {**table, **out}.items()})


if __name__ == "__main__":
    main()
