"""One ``TAGConv`` layer + leaky ReLU (``gn_tag_propagate`` + ``gn_tagconv_fwd`` forward, Horner backward) against float64
autograd over the operands as the kernels see them: in bf16 mode the weights and the staged ``[x | h1 | h2]`` operand are
rounded to bf16, straight-through for the gradient, so that the reference takes the same leaky decisions
(gates as ``tests/test_gpu_leaky.py``: fp32 1e-4 forward / 1e-3 gradients; bf16 2e-2 max-norm and Frobenius)."""
import pytest
import torch

from tagconv_reference import dense_p, make_batch, norm_err, rel_err

pytestmark = pytest.mark.gpu


# (256, 64, fp32) is the widest A tile (above 64 KB of LDS)
@pytest.mark.parametrize("cin,cout,dtype,K", [(ci, co, dt, K) for ci, co in [(32, 128), (128, 128)] for dt in ["fp32", "bf16"]
                                              for K in [8, 16]] + [(256, 64, "fp32", 8)])
def test_layer_forward_and_gradients(cin, cout, dtype, K):
    from graphnet_amd import TAGConv, ops
    lowp = dtype == "bf16"
    ei, _, _, N = make_batch(K)
    P = dense_p(ei, N)
    torch.manual_seed(cin + cout + K)
    conv = TAGConv(cin, cout).cuda()
    with torch.no_grad():
        conv.bias.normal_(0, 0.1)
    x = torch.randn(N, cin, device="cuda", requires_grad=True)
    gout = torch.randn(N, cout, device="cuda")
    out = conv(x, ops.table_from_edge_index(ei.cuda(), N, K), mode=ops.MODE_BF16 if lowp else ops.MODE_F32)
    out.backward(gout)

    def rnd(t):
        return t + (t.float().bfloat16().double() - t).detach() if lowp else t
    xd = x.detach().double().cpu().requires_grad_()
    Wd = [l.weight.detach().double().cpu().requires_grad_() for l in conv.lins]
    bd = conv.bias.detach().double().cpu().requires_grad_()
    h1 = P @ xd
    pre = sum(rnd(h) @ rnd(W).t() for h, W in zip([xd, h1, P @ h1], Wd)) + bd
    ref = torch.nn.functional.leaky_relu(pre, 0.01)
    ref.backward(gout.double().cpu())
    pairs = [("dx", x.grad, xd.grad), ("db", conv.bias.grad, bd.grad)] + \
            [(f"dW{k}", conv.lins[k].weight.grad, Wd[k].grad) for k in range(3)]
    e_out = rel_err(out, ref), norm_err(out, ref)
    e_grad = {n: (rel_err(a, b), norm_err(a, b)) for n, a, b in pairs}
    print("out", e_out, "grads", e_grad)
    if lowp:
        assert max(e_out) < 2e-2 and all(max(e) < 2e-2 for e in e_grad.values())
    else:
        assert e_out[0] < 1e-4 and all(e[0] < 1e-3 for e in e_grad.values())
