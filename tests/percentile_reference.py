"""Plain restatement of the ``gn_percentile_clusters`` contract (``include/graphnet_amd.h``): one Python loop per cluster,
one per percentile.  Written from the contract and kept apart from the product's vectorised host path
(``graphnet_amd.graphs.percentile_clusters_host``), which the tests compare against it."""
import math

import numpy as np

NAN_KEY = 0xFFFFFFFF


def cluster_key(v) -> int:
    """Key of a cluster value: fp32 bits, -0.0 as +0.0, every NaN one key after +inf, then the order-preserving map."""
    v = np.float32(v)
    if np.isnan(v):
        return NAN_KEY
    if v == 0:
        v = np.float32(0.0)
    b = int(np.array([v], dtype=np.float32).view(np.uint32)[0])
    return (~b & 0xFFFFFFFF) if b >> 31 else (b | 0x80000000)


def linear_percentile(v, q: float) -> np.float32:
    """``v``: ascending non-NaN values as Python floats (fp64), ``q`` in [0, 1]."""
    m = len(v)
    if m == 0:
        return np.float32(np.nan)
    h = (m - 1) * q
    lo = math.floor(h)
    hi = min(lo + 1, m - 1)
    g = h - lo
    a, b = v[lo], v[hi]
    d = b - a
    r = b - d * (1 - g) if g >= 0.5 else a + d * g
    with np.errstate(over="ignore"):
        return np.float32(r)


def cluster_event(x, cluster_cols, summ_cols, percentiles, add_counts=True):
    """fp32 ``[n, F]`` of ONE event -> ``(nodes fp32 [M, W], members)``; ``members[r]`` = pulse indices of node r."""
    x = np.asarray(x, dtype=np.float32)
    groups = {}
    for i in range(len(x)):
        # most significant key: the LAST cluster column
        groups.setdefault(tuple(cluster_key(x[i, c]) for c in reversed(cluster_cols)), []).append(i)
    W = len(cluster_cols) + len(summ_cols) * len(percentiles) + (1 if add_counts else 0)
    rows, members = [], []
    for key in sorted(groups):
        idx = groups[key]
        row = [x[idx[0], c] for c in cluster_cols]
        for f in summ_cols:
            vals = x[idx, f]
            v = [float(t) for t in np.sort(vals[~np.isnan(vals)])]
            row += [linear_percentile(v, float(np.float64(p) / 100)) for p in percentiles]
        if add_counts:
            row.append(np.float32(np.log10(np.float64(len(idx)))))
        rows.append(row)
        members.append(idx)
    return np.asarray(rows, dtype=np.float32).reshape(len(rows), W), members


def cluster_batch(x, ptr, cluster_cols, summ_cols, percentiles, add_counts=True):
    """``(nodes fp32 [M, W], node_ptr int32 [B + 1])`` of a flat batch."""
    x = np.asarray(x, dtype=np.float32)
    ptr = [int(v) for v in ptr]
    parts = [cluster_event(x[lo:hi], cluster_cols, summ_cols, percentiles, add_counts)[0] for lo, hi in zip(ptr[:-1], ptr[1:])]
    W = len(cluster_cols) + len(summ_cols) * len(percentiles) + (1 if add_counts else 0)
    nodes = np.concatenate(parts, axis=0) if parts else np.zeros((0, W), dtype=np.float32)
    return nodes, np.cumsum([0] + [len(p) for p in parts]).astype(np.int32)


def same(a, b) -> bool:
    """Equal entry for entry, NaN == NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


def same_but_counts(got, exp, add_counts=True) -> bool:
    """Device output against host output: exact, but for the counts column, where the device ``log10`` may land on the
    adjacent fp32 value (bit patterns at most 1 apart; exactly 0.0 for a single pulse)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if not add_counts:
        return same(got, exp)
    if got.shape != exp.shape or got.dtype != np.float32 or exp.dtype != np.float32:
        return False
    gc, ec = np.ascontiguousarray(got[:, -1]).view(np.int32).astype(np.int64), np.ascontiguousarray(exp[:, -1]).view(np.int32).astype(np.int64)
    return same(got[:, :-1], exp[:, :-1]) and bool((np.abs(gc - ec) <= 1).all()) and bool((gc[ec == 0] == 0).all())


# ---- the inputs that the host file and the GPU file share -------------------------------------------------------------
def make_event(gen, n, F=6, dup=4):
    pos = gen.standard_normal((max(1, n // dup), 3)).astype(np.float32)
    return np.concatenate([pos[gen.integers(0, len(pos), n)],
                           gen.standard_normal((n, F - 3)).astype(np.float32)], 1)


SIZES = [1, 2, 3, 9, 63, 64, 65, 256, 257, 600, 1100, 2049]


def shapes_batch():
    gen = np.random.default_rng(20)
    events = [make_event(gen, n) for n in SIZES]
    return np.concatenate(events, axis=0), np.cumsum([0] + SIZES)


def grid_event(cluster_nan=False):
    """Integer-grid positions (many ties), ``-0.0`` beside ``+0.0``, forty coincident pulses, NaN and +-inf in summarised
    columns; ``cluster_nan``: also NaNs in cluster columns."""
    gen = np.random.default_rng(5)
    n = 300
    x = np.concatenate([gen.integers(-1, 3, (n, 3)).astype(np.float32), gen.standard_normal((n, 3)).astype(np.float32)], 1)
    x[gen.random(n) < 0.5, 0] *= np.float32(-1.0)            # 0 -> -0.0 for half of the zeros (and 1 <-> -1)
    x[40:80, :3] = x[40, :3]
    x[45, 3] = np.nan
    x[50:53, 4] = np.nan
    x[7, 3] = np.nan
    x[60, 5] = np.inf
    x[61, 5] = -np.inf
    x[100, 4] = np.inf
    same_dom = np.flatnonzero((x[:, :3] == x[3, :3]).all(1))
    x[same_dom, 5] = np.nan                                   # a cluster whose every value of a column is NaN
    if cluster_nan:
        x[[9, 120, 250], :2] = [1.0, 2.0]
        x[[9, 250], 2] = np.nan
        x[120:121, 2].view(np.uint32)[:] = 0xFFC00123        # another NaN: sign and payload bits set
    return x
