"""Regenerates ``percentile_clusters_expected.npz``: what the REFERENCE's ``cluster_summarize_with_percentiles`` returns on
bundled events (``reference_events.npz`` cast to fp32), cast to fp32.  Only the recorded numbers are stored.

    python tests/golden/make_percentile_fixtures.py <path to the reference's models/graphs/utils.py>

The module itself pulls in packages that this project does not need, so the three function definitions the recipe uses
are taken out of its syntax tree at run time and executed against numpy alone.
"""
import ast
import os
import sys
from typing import List, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
WANTED = ("lex_sort", "gather_cluster_sequence", "cluster_summarize_with_percentiles")
# dataset -> (number of events stored, percentiles); clustered on columns 0-2, counts added
CASES = {"prometheus": (50, [0, 10, 50, 90, 100]), "deepcore": (5, [0, 10, 50, 90, 100]), "upgrade": (2, [0, 50, 100])}


def reference_functions(utils_py: str) -> dict:
    tree = ast.parse(open(utils_py).read())
    body = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    assert sorted(f.name for f in body) == sorted(WANTED)
    ns = {"np": np, "List": List, "Tuple": Tuple}
    exec(compile(ast.Module(body=body, type_ignores=[]), utils_py, "exec"), ns)
    return ns


def main() -> None:
    summarize = reference_functions(sys.argv[1])["cluster_summarize_with_percentiles"]
    ev = np.load(os.path.join(HERE, "reference_events.npz"))
    out = {}
    for name, (count, percentiles) in CASES.items():
        x, ptr = ev[name + "_x"].astype(np.float32), ev[name + "_ptr"]
        cluster, summ = [0, 1, 2], list(range(3, x.shape[1]))
        rows = [summarize(x[ptr[i]:ptr[i + 1]], summ, cluster, percentiles, True).astype(np.float32) for i in range(count)]
        out[name + "_nodes"] = np.concatenate(rows, axis=0)
        out[name + "_node_ptr"] = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
        out[name + "_percentiles"] = np.asarray(percentiles, dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "percentile_clusters_expected.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
