"""numpy fp32 brute force of the ``RadialEdges`` / ``gn_radius_graph`` contract: the expected table of the radius tests.

numpy's elementwise fp32 operations do not fuse, so this is the contract bit for bit::

    d2 = ((0 + e0*e0) + e1*e1) + ...     e = x[j, col] - x[i, col], columns left to right
    r2 = fp32(r) * fp32(r)
    edge j -> i   iff   j != i  and  d2 < r2        (strict; a NaN or inf d2 fails it)

Sources ascend by ``j``; a centre with more than ``cap`` in-radius pulses keeps the ``cap`` smallest ``(d2, j)``, still
ascending by ``j``.  ``tests/test_radial_host.py`` pins it against ``scipy.spatial.cKDTree``."""
import numpy as np
import torch


def ptr_of(sizes):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor(sizes, dtype=torch.int64), 0)
    return ptr


def radius_table(x, ptr, cols, r, cap):
    """``(nbr[N, cap] int32 -1 padded, deg[N] int32 uncapped)`` of a CPU ``x`` with event offsets ``ptr``."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    ptr = np.asarray(ptr.cpu().numpy() if isinstance(ptr, torch.Tensor) else ptr)
    N = x.shape[0]
    r2 = np.float32(r) * np.float32(r)
    nbr = np.full((N, cap), -1, np.int32)
    deg = np.zeros(N, np.int32)
    for b in range(len(ptr) - 1):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        n = hi - lo
        if n < 1:
            continue
        d2 = np.zeros((n, n), np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for c in cols:
                v = x[lo:hi, c]
                diff = v[None, :] - v[:, None]                    # candidate - centre
                d2 = d2 + diff * diff
            inr = d2 < r2
        inr[np.arange(n), np.arange(n)] = False
        for i in range(n):
            js = np.nonzero(inr[i])[0]
            deg[lo + i] = len(js)
            if len(js) > cap:
                order = np.lexsort((js, d2[i, js]))               # (d2, j)
                js = np.sort(js[order[:cap]])
            nbr[lo + i, :len(js)] = js + lo
    return torch.from_numpy(nbr), torch.from_numpy(deg)


def edge_index_of(nbr):
    n, w = nbr.shape
    centre = torch.arange(n, dtype=torch.int64).unsqueeze(1).expand(n, w)
    valid = nbr >= 0
    return torch.stack([nbr[valid].to(torch.int64), centre[valid]], dim=0)
