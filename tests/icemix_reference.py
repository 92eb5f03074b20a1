"""Plain restatement of the ``gn_icemix_nodes`` contract (``include/graphnet_amd.h``), written from the header: the hash in
Python integers / uint64 numpy, one Python loop per event, and the ice interpolation one pulse at a time in Python floats
(fp64, one rounding per operation, no fused multiply-add).  Shares no code with the package.
"""
import bisect
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M32 = 0xFFFFFFFF


def mix32(v):
    """``gn_mix32`` on uint32 values held in Python ints or uint64 arrays."""
    v = v ^ (v >> 16)
    v = (v * 0x21F0AAAD) & M32
    v = v ^ (v >> 15)
    v = (v * 0x735A2D97) & M32
    return v ^ (v >> 15)


def keys(seed, event_id, n, key_bits=32):
    """uint64 ``[..., n]``: the key of pulses 0..n-1; ``seed`` and ``event_id`` broadcast against each other."""
    seed = np.asarray(seed, dtype=np.uint64) & np.uint64(M32)
    e = np.asarray(event_id, dtype=np.uint64) & np.uint64(M32)
    stream = mix32(seed ^ ((e * np.uint64(0x9E3779B1)) & np.uint64(M32)))
    i = np.arange(n, dtype=np.uint64)
    return mix32(stream[..., None] ^ ((i * np.uint64(0x85EBCA77)) & np.uint64(M32))) >> np.uint64(32 - key_bits)


def kept(seed, event_id, n, L, key_bits=32):
    """Ascending pulse indices of one event: all of them for ``n <= L``, else pulse i iff fewer than L pulses precede it in
    the total order (key, index)."""
    if n <= L:
        return list(range(n))
    h = [int(v) for v in keys(seed, event_id, n, key_bits)]
    order = sorted(range(n), key=lambda i: (h[i], i))
    return sorted(order[:L])


def kept_many(seeds, event_ids, n, L):
    """bool ``[draws, n]``: which pulses every draw keeps (n > L, 32 key bits)."""
    h = keys(seeds, event_ids, n)
    order = np.argsort(h, axis=-1, kind="stable")                 # ties (never seen at 32 bits) by index
    mask = np.zeros(h.shape, dtype=bool)
    np.put_along_axis(mask, order[:, :L], True, axis=-1)
    return mask


def load_table(prefix="d_"):
    """fp64 ``[3, T]`` (knots, scattering, absorption) as the reference's ``ice_transparency`` built it (recorded)."""
    d = np.load(os.path.join(GOLDEN, "icemix_nodes_expected.npz"))
    return np.stack([d[prefix + "z_norm"], d[prefix + "scatt"], d[prefix + "abs"]])


def ice(table, zf):
    """``(scattering, absorption)`` as fp32 for ONE fp32 depth; NaN in both outside the table."""
    zt, ys, ya = (row.tolist() for row in table)
    z = float(np.float32(zf))
    if not (z >= zt[0] and z <= zt[-1]):
        return np.float32(np.nan), np.float32(np.nan)
    j = min(bisect.bisect_right(zt, z) - 1, len(zt) - 2)
    out = []
    for y in (ys, ya):
        slope = (y[j + 1] - y[j]) / (zt[j + 1] - zt[j])
        prod = slope * (z - zt[j])
        out.append(np.float32(prod + y[j]))
    return tuple(out)


def nodes_batch(x, ptr, L, hlc_col=-1, z_col=-1, table=None, seed=0, event_ids=None, key_bits=32):
    """``(out fp32 [M, W], out_ptr int32 [B + 1], ids int32 [M])`` of the contract."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F = x.shape[1]
    W = F + (2 if z_col >= 0 else 0)
    rows, ids, out_ptr = [], [], [0]
    for b in range(len(ptr) - 1):
        lo, n = int(ptr[b]), int(ptr[b + 1]) - int(ptr[b])
        for i in kept(seed, b if event_ids is None else int(event_ids[b]), n, L, key_bits):
            row = np.zeros(W, dtype=np.float32)
            row[:F] = x[lo + i]
            if hlc_col >= 0:
                row[hlc_col] = 1.0 if x[lo + i, hlc_col] == 0 else 0.0
            if z_col >= 0:
                row[F], row[F + 1] = ice(table, x[lo + i, z_col])
            rows.append(row)
            ids.append(lo + i)
        out_ptr.append(len(ids))
    out = np.stack(rows) if rows else np.zeros((0, W), dtype=np.float32)
    return out, np.asarray(out_ptr, dtype=np.int32), np.asarray(ids, dtype=np.int32)


def same(a, b):
    """Bit for bit, every NaN equal to every NaN."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def shapes_batch(F, rng, sizes=(0, 2, 63, 64, 65, 131, 5000)):
    """fp32 ``[N, F]`` with column 2 a depth inside the default table (every seventh one the fp32 number next to a knot, the
    two ends of the table included; no knot of this table is an fp32 number itself), column F - 1 an hlc-like flag with
    0, 1, -0.0, 2 and NaN, the rest normal draws; and ``ptr``."""
    zt = load_table()[0]
    N = int(sum(sizes))
    x = rng.standard_normal((N, F)).astype(np.float32)
    z = rng.uniform(zt[0], zt[-1], N).astype(np.float32)
    z[::7] = zt[np.arange(len(z[::7])) % len(zt)].astype(np.float32)
    z = np.where(z.astype(np.float64) < zt[0], np.nextafter(z, np.float32(np.inf)), z)
    z = np.where(z.astype(np.float64) > zt[-1], np.nextafter(z, np.float32(-np.inf)), z)
    assert ((z.astype(np.float64) >= zt[0]) & (z.astype(np.float64) <= zt[-1])).all()
    x[:, 2] = z
    x[:, F - 1] = rng.choice(np.asarray([0.0, 1.0, -0.0, 2.0, np.nan], dtype=np.float32), N)
    return x, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
