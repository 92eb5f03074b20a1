"""Readable restatements for the DOM time series tests (no product code):

* :func:`event_rows` / :func:`series_batch` - the ``gn_dom_time_series`` contract (``include/graphnet_amd.h``), one event
  and one DOM at a time;
* :func:`gru_reference` - the reference's own call (``models/rnn/node_rnn.py:105-111``): ``torch.nn.GRU`` in float64 on the
  CPU over ``pack_sequence(enforce_sorted=False)``, output ``[-1][0]``;
* :func:`dom_rows_reference` - ``node_rnn.py:113-122`` in float64.
"""
import math

import numpy as np
import torch


def _key(v):
    """Sort key of an id or time value: -0.0 as +0.0, every NaN one value after +inf."""
    v = float(v)
    return (1, 0.0) if math.isnan(v) else (0, v + 0.0)


def event_rows(x, id_cols, time_col, charge_col=-1):
    """fp32 ``[n, F]`` -> (fp32 ``[n, W]``, list of series lengths), W = F + (charge_col < 0) + 1."""
    x = np.asarray(x, dtype=np.float32)
    n, F = x.shape
    W = F + (1 if charge_col < 0 else 0) + 1
    order = sorted(range(n), key=lambda i: (tuple(_key(x[i, c]) for c in reversed(id_cols)), _key(x[i, time_col]), i))
    tmin = np.float32(np.inf)
    for i in range(n):
        t = x[i, time_col]
        if np.isnan(t) or np.isnan(tmin):
            tmin = np.float32(np.nan)
        elif t < tmin or (t == tmin and np.signbit(t)):         # -0.0 before +0.0
            tmin = t
    doms = []                                                   # pulses of every DOM, in order
    for i in order:
        ident = tuple(_key(x[i, c]) for c in id_cols)
        if not doms or doms[-1][0] != ident:
            doms.append((ident, []))
        doms[-1][1].append(i)
    out = np.empty((n, W), dtype=np.float32)
    r = 0
    with np.errstate(over="ignore", invalid="ignore"):
        for _, pulses in doms:
            for j, i in enumerate(pulses):
                out[r, :F] = x[i]
                out[r, time_col] = np.float32(x[i, time_col] - tmin)
                if charge_col < 0:
                    out[r, F] = 1.0
                else:
                    out[r, charge_col] = np.float32(np.power(np.float64(10.0), np.float64(x[i, charge_col])))
                out[r, W - 1] = 1.0 if j == 0 else 0.0
                r += 1
    return out, [len(p) for _, p in doms]


def series_batch(x, ptr, id_cols, time_col, charge_col=-1):
    """Every event of the batch: ``(rows [N, W], series_ptr int32 [M + 1], dom_ptr int32 [B + 1], longest series)``."""
    parts, lengths, dom_ptr = [], [], [0]
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        rows, lens = event_rows(x[lo:hi], id_cols, time_col, charge_col)
        parts.append(rows)
        lengths += lens
        dom_ptr.append(dom_ptr[-1] + len(lens))
    W = x.shape[1] + (1 if charge_col < 0 else 0) + 1
    rows = np.concatenate(parts, axis=0) if parts else np.zeros((0, W), dtype=np.float32)
    series_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rows, series_ptr, np.asarray(dom_ptr, dtype=np.int32), max(lengths) if lengths else 0


def same(a, b):
    """Equal entry for entry, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def ulp_distance(a, b):
    """Largest distance in fp32 units in the last place between two arrays of non-negative values (inf and NaN must match)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    special = ~np.isfinite(a) | ~np.isfinite(b)
    assert same(a[special], b[special])
    d = np.abs(a[~special].view(np.int32).astype(np.int64) - b[~special].view(np.int32).astype(np.int64))
    return int(d.max()) if d.size else 0


def same_but_charge(got, exp, charge_col, ulps=1):
    """Exact everywhere, but the charge column may differ by ``ulps`` fp32 bit patterns (another libm's ``pow``)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return False
    if charge_col < 0:
        return same(got, exp)
    keep = [c for c in range(got.shape[1]) if c != charge_col]
    return same(got[:, keep], exp[:, keep]) and ulp_distance(got[:, charge_col], exp[:, charge_col]) <= ulps


def shapes_batch(lds_max=4096, seed=5):
    """One batch of the shapes where the kernel can go wrong: fp32 ``[N, 6]`` = x, y, z, t, log10 charge, one more column.
    Events of 2, 3 and 64 pulses; 40 pulses on one DOM; 40 pulses on 40 DOMs; 511, 512, 513 pulses; ``lds_max`` and
    ``lds_max + 1`` pulses.  Times are whole numbers from a small range, so a DOM often sees equal times."""
    rng = np.random.default_rng(seed)
    sizes = [2, 3, 64, 40, 40, 511, 512, 513, lds_max, lds_max + 1]
    events = []
    for e, n in enumerate(sizes):
        n_dom = 1 if e == 3 else max(2, n // 6)
        grid = rng.integers(-5, 6, size=(n_dom, 3)).astype(np.float32) * 17.0
        pick = np.arange(n) if e == 4 else rng.integers(0, n_dom, size=n)
        if e == 4:
            grid = np.stack([np.arange(n), np.arange(n) % 3, np.arange(n) % 5], axis=1).astype(np.float32)
        ev = np.empty((n, 6), dtype=np.float32)
        ev[:, :3] = grid[pick]
        ev[:, 3] = rng.integers(0, 12, size=n).astype(np.float32) + 9000.0
        ev[:, 4] = rng.normal(0.0, 0.5, size=n).astype(np.float32)
        ev[:, 5] = rng.normal(size=n).astype(np.float32)
        events.append(ev[rng.permutation(n)])
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.concatenate(events, axis=0), ptr


def gru_reference(xs, series_ptr, params, num_layers=1):
    """``(out float64 [M, H], gru)``: ``torch.nn.GRU`` in float64 on the CPU, literally the reference's call.  ``params``:
    name -> tensor for ``weight_ih_l0`` ...; ``out`` is attached to ``gru``'s parameters for a backward pass."""
    I, H = int(params["weight_ih_l0"].shape[1]), int(params["weight_hh_l0"].shape[1])
    gru = torch.nn.GRU(num_layers=num_layers, input_size=I, hidden_size=H, batch_first=True).double()
    with torch.no_grad():
        for name, p in gru.named_parameters():
            p.copy_(params[name].detach().double().cpu())
    xs64 = torch.as_tensor(np.asarray(xs), dtype=torch.float64)
    sp = [int(v) for v in series_ptr]
    packed = torch.nn.utils.rnn.pack_sequence([xs64[a:b] for a, b in zip(sp[:-1], sp[1:])], enforce_sorted=False)
    return gru(packed)[-1][0], gru


def dom_rows_reference(x, series_ptr, charge_col):
    """float64 ``[M, F]``: every series' first row without ``new_node_col``, the charge column replaced by
    ``asinh(5 * sum / 5)`` of the series' charges."""
    x = np.asarray(x, dtype=np.float64)
    sp = [int(v) for v in series_ptr]
    out = x[sp[:-1], :-1].copy()
    for s, (a, b) in enumerate(zip(sp[:-1], sp[1:])):
        out[s, charge_col] = np.arcsinh(5.0 * x[a:b, charge_col].sum() / 5.0)
    return out
