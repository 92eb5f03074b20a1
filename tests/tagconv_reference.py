"""Shared by the TAGConv / ConvNet GPU tests: one small hand-made batch and the dense float64 propagation matrix.

Events (161 nodes = 5 tiles of 32 centres + 1): 1 node (no edge); 2 nodes with the single edge 0 -> 1 (a source of degree 0);
40 nodes where centre i has i % (K + 2) in-edges (rows shorter than K, full rows, and K + 1 = an overflow entry); 100 nodes
that all receive from node 0 of the event (a reverse list of 99 rows: the hub branch) and from their successor; 18 nodes
on a ring."""
import torch

SIZES = [1, 2, 40, 100, 18]


def make_batch(K):
    src, dst, off = [], [], 0
    for e, n in enumerate(SIZES):
        for i in range(n):
            if e == 1:
                nb = [0] if i == 1 else []
            elif e == 2:
                nb = [(i + 1 + d) % n for d in range(i % (K + 2))]
            elif e == 3:
                nb = [] if i == 0 else [0] + ([(i + 1) % n] if (i + 1) % n else [])
            else:
                nb = [(i + 1) % n, (i + 2) % n] if n > 2 else []
            src += [off + j for j in nb]
            dst += [off + i] * len(nb)
        off += n
    ptr = torch.tensor([0] + SIZES).cumsum(0)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    return torch.tensor([src, dst], dtype=torch.int64), ptr, batch, off


def dense_p(ei, N):
    """P[i, j] = dis[i] dis[j] per edge j -> i, dis = deg^-1/2 of the in-degree (0 where deg == 0), float64."""
    deg = torch.bincount(ei[1], minlength=N).double()
    dis = torch.where(deg > 0, deg.clamp_min(1).rsqrt(), torch.zeros_like(deg))
    P = torch.zeros(N, N, dtype=torch.float64)
    P.index_put_((ei[1], ei[0]), dis[ei[1]] * dis[ei[0]], accumulate=True)
    return P


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def norm_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))
