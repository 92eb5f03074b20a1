"""Regenerates ``dom_time_series_expected.npz``: what the REFERENCE's ``NodeAsDOMTimeSeries._construct_nodes`` returns on
bundled events (``reference_events.npz`` cast to fp32, the charge column passed through fp32 ``log10`` first - it is stored
raw, and ``10^x`` of a raw charge overflows), cast to fp32.  The inputs as fed and the recorded outputs are stored: numbers only.

    python tests/golden/make_dom_series_fixtures.py <the reference's models/graphs/utils.py> <its models/graphs/nodes/nodes.py>

The modules pull in packages that this project does not need, so ``lex_sort`` and the method's definition are taken out of
their syntax trees at run time and executed against numpy alone (``torch.tensor`` and ``Data`` become pass-throughs).
"""
import ast
import os
import sys
import types
from typing import List, Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# case -> (dataset, number of events stored, keys, charge_column); ids are columns 0-2, time is column 3
CASES = {
    "prometheus": ("prometheus", 50, ["x", "y", "z", "t"], "None"),           # the example: no charge column
    "deepcore": ("deepcore", 5, None, "charge"),
    "upgrade": ("upgrade", 2, None, "charge"),
    "deepcore_none": ("deepcore", 5, None, "None"),
}
CHARGE = 4


def reference_method(utils_py: str, nodes_py: str):
    tree = ast.parse(open(utils_py).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "lex_sort"]
    cls = [n for n in ast.parse(open(nodes_py).read()).body if isinstance(n, ast.ClassDef) and n.name == "NodeAsDOMTimeSeries"]
    body += [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "_construct_nodes"]
    assert [f.name for f in body] == ["lex_sort", "_construct_nodes"]
    ns = {"np": np, "List": List, "Optional": Optional, "Data": lambda x: x,
          "torch": types.SimpleNamespace(tensor=lambda a: a, Tensor=object)}
    exec(compile(ast.Module(body=body, type_ignores=[]), nodes_py, "exec"), ns)
    return ns["_construct_nodes"]


class _Pulses:
    def __init__(self, a: np.ndarray):
        self._a = a

    def numpy(self) -> np.ndarray:
        return self._a.copy()


def main() -> None:
    construct = reference_method(sys.argv[1], sys.argv[2])
    ev = np.load(os.path.join(HERE, "reference_events.npz"))
    out = {}
    for case, (name, count, keys, charge_column) in CASES.items():
        x, ptr = ev[name + "_x"].astype(np.float32), ev[name + "_ptr"][:count + 1]
        x = x[:ptr[-1]].copy()
        if x.shape[1] > CHARGE:
            assert (x[:, CHARGE] > 0).all()
            x[:, CHARGE] = np.log10(x[:, CHARGE])
        keys = keys or ["x", "y", "z", "t", "charge"] + [f"f{i}" for i in range(5, x.shape[1])]
        me = types.SimpleNamespace(_keys=keys, _id_columns=[0, 1, 2], _time_index=3,
                                   _charge_index=keys.index(charge_column) if charge_column in keys else None)
        rows = [np.asarray(construct(me, _Pulses(x[ptr[i]:ptr[i + 1]]))).astype(np.float32) for i in range(count)]
        out[case + "_x"] = x
        out[case + "_ptr"] = ptr.astype(np.int32)
        out[case + "_rows"] = np.concatenate(rows, axis=0)
        out[case + "_charge_col"] = np.asarray(-1 if me._charge_index is None else me._charge_index, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "dom_time_series_expected.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
