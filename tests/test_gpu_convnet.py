"""``ConvNet(7, 3, nb_intermediate=64, dropout_ratio=0.0)`` in fp32 mode against a float64 restatement of the reference's
``ConvNet.forward`` from plain torch ops: output, every parameter gradient, the running statistics (train mode) and eval
mode; gates 1e-4 forward / 1e-3 gradients.  The restatement has the reference's state-dict layout, so loading its weights
is the round-trip check."""
import types

import pytest
import torch

from tagconv_reference import make_batch, rel_err

pytestmark = pytest.mark.gpu


class _RefTAG(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.lins = torch.nn.ModuleList([torch.nn.Linear(cin, cout, bias=False) for _ in range(3)])
        self.bias = torch.nn.Parameter(0.1 * torch.randn(cout))

    def forward(self, x, ei, w):
        out, h = self.lins[0](x) + self.bias, x
        for lin in self.lins[1:]:
            h = torch.zeros_like(h).index_add(0, ei[1], h[ei[0]] * w[:, None])
            out = out + lin(h)
        return out


class _RefConvNet(torch.nn.Module):
    def __init__(self, nin, nout, c):
        super().__init__()
        self.conv1, self.conv2, self.conv3 = _RefTAG(nin, c), _RefTAG(c, c), _RefTAG(c, c)
        self.batchnorm1 = torch.nn.BatchNorm1d(6 * c)
        for l in range(1, 6):
            setattr(self, f"linear{l}", torch.nn.Linear(6 * c, 6 * c))
        self.out = torch.nn.Linear(6 * c, nout)

    def forward(self, x, ei, batch, B):
        deg = torch.bincount(ei[1], minlength=x.shape[0]).to(x.dtype)
        dis = torch.where(deg > 0, deg.clamp_min(1).rsqrt(), torch.zeros_like(deg))
        w, pooled = dis[ei[0]] * dis[ei[1]], []
        for conv in (self.conv1, self.conv2, self.conv3):
            x = torch.nn.functional.leaky_relu(conv(x, ei, w))
            pooled += [torch.zeros(B, x.shape[1], dtype=x.dtype).index_add(0, batch, x),
                       torch.stack([x[batch == b].amax(0) for b in range(B)])]
        x = self.batchnorm1(torch.cat(pooled, dim=1))
        for l in range(1, 6):
            x = torch.nn.functional.leaky_relu(getattr(self, f"linear{l}")(x))
        return self.out(x)


@pytest.mark.parametrize("train", [True, False])
def test_convnet_matches_float64_restatement(train):
    from graphnet_amd import ConvNet
    torch.manual_seed(3)
    ei, ptr, batch, N = make_batch(8)
    B = len(ptr) - 1
    ref = _RefConvNet(7, 3, 64)
    with torch.no_grad():
        ref.batchnorm1.running_mean.normal_()
        ref.batchnorm1.running_var.uniform_(0.5, 2.0)
    model = ConvNet(7, 3, nb_intermediate=64, dropout_ratio=0.0).set_backend(dtype="fp32")
    model.load_state_dict(ref.state_dict())
    assert list(model.state_dict()) == list(ref.state_dict())
    assert all(torch.equal(v, ref.state_dict()[k]) for k, v in model.state_dict().items())
    model, ref = model.cuda().train(train), ref.double().train(train)
    x, gout = torch.randn(N, 7), torch.randn(B, 3)
    data = types.SimpleNamespace(x=x.cuda(), edge_index=ei.cuda(), batch=batch.cuda(), ptr=ptr.cuda())
    out = model(data)
    out.backward(gout.cuda())
    want = ref(x.double(), ei, batch, B)
    want.backward(gout.double())
    grads, want_grads = dict(model.named_parameters()), dict(ref.named_parameters())
    e_out = rel_err(out, want)
    e_grad = {k: rel_err(grads[k].grad, want_grads[k].grad) for k in want_grads}
    e_stat = max(rel_err(getattr(model.batchnorm1, s), getattr(ref.batchnorm1, s)) for s in ("running_mean", "running_var"))
    print("out", e_out, "stats", e_stat, "grads", e_grad)
    assert e_out < 1e-4 and e_stat < 1e-4 and all(e < 1e-3 for e in e_grad.values())
