"""``gn_tag_propagate`` / ``gn_tag_propagate_t`` against the dense float64 P of the same ``edge_index``.

Gate 1e-5 of max|ref|: a sum of at most 33 products plus three scalings accumulates about 36 fp32 roundings (2.2e-6); the
inputs are standard normal, so the absolute sum is within a small factor of the maximum - the gate leaves about 4x."""
import pytest
import torch

from tagconv_reference import dense_p, make_batch, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("C", [32, 128])
def test_propagate_and_transpose_match_dense_p(C, K):
    from graphnet_amd import ops
    ei, _, _, N = make_batch(K)
    P = dense_p(ei, N)
    g = ops.table_from_edge_index(ei.cuda(), N, K)
    assert g.K == K and int(g.ovf_cnt.item()) > 0                      # the K + 1 rows went to the overflow column
    dis = ops.tag_norm(g)
    gen = torch.Generator().manual_seed(C + K)
    x, gr, add = (torch.randn(N, C, generator=gen) for _ in range(3))
    h = ops.tag_propagate(x.cuda(), C, g, dis)
    t = ops.tag_propagate_t(gr.cuda(), C, g, dis, add=add.cuda())
    assert int(g.rev_nhubs[0].item()) >= 1                              # the 99-row reverse list ran on the hub kernel
    errs = rel_err(h, P @ x.double()), rel_err(t, P.T @ gr.double() + add.double())
    print("rel err", errs)
    assert max(errs) < 1e-5
    assert torch.equal(h, ops.tag_propagate(x.cuda(), C, g, dis))
    assert torch.equal(t, ops.tag_propagate_t(gr.cuda(), C, g, dis, add=add.cuda()))
