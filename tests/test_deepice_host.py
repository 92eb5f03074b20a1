"""Host-side tests of ``DeepIce`` (no GPU): state-dict compatibility with the restatement of the reference
(``tests/deepice_reference.py``), config round trip, the ``IceCubeKaggle`` detector, and the identity the biased attention
kernel rests on (dense bias tensor == factored form) in float64."""
import numpy as np
import pytest
import torch

import deepice_reference as ref

SMALL = dict(hidden_dim=64, head_size=32, seq_length=32, depth=2, depth_rel=2)
DYNEDGE_ARGS = dict(nb_inputs=6, nb_neighbours=9, post_processing_layer_sizes=[48, 32], dynedge_layer_sizes=[(32, 48), (48, 32)],
                    global_pooling_schemes=None, activation_layer="gelu", add_norm_layer=True, skip_readout=True)


def _shapes(module):
    return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]


@pytest.mark.parametrize("kw", [
    {}, {"include_dynedge": True}, {"scaled_emb": True}, {"n_features": 4}, {"n_features": 5}, {"n_features": 6},
    {"include_dynedge": True, "dynedge_args": DYNEDGE_ARGS},
], ids=lambda kw: "-".join(f"{k}={v if not isinstance(v, dict) else 'given'}" for k, v in kw.items()) or "defaults")
def test_state_dict_matches_the_restatement(kw):
    """Keys, their order and shapes; ``load_state_dict`` in both directions.  (Small widths except for the defaults and
    the default embedded DynEdge, whose sizes are the point.)"""
    import graphnet_amd as g
    kw = dict(kw) if not kw or kw == {"include_dynedge": True} else dict(SMALL, **kw)
    torch.manual_seed(0)
    theirs = ref.DeepIce(**kw)
    ours = g.DeepIce(**kw)
    assert _shapes(ours) == _shapes(theirs)
    ours.load_state_dict(theirs.state_dict())
    for (k, a), (_, b) in zip(ours.state_dict().items(), theirs.state_dict().items()):
        assert torch.equal(a, b), k
    torch.manual_seed(1)
    again = g.DeepIce(**kw)
    theirs.load_state_dict(again.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(theirs.state_dict().values(), again.state_dict().values()))
    names = [k for k, _ in ours.named_parameters()]
    assert "cls_token.weight" in names and "rel_pos.projection.weight" in names
    assert not any("gamma" in k for k in names if k.startswith("sandwich."))
    assert all(f"blocks.{i}.gamma_1" in names and f"blocks.{i}.attn.in_proj_weight" in names for i in range(len(ours.blocks)))
    assert ("fourier_ext.sin_emb.scale" in names) == bool(kw.get("scaled_emb"))
    assert ("fourier_ext.aux_emb.weight" in names) == (kw.get("n_features", 6) >= 6)
    assert any(k.startswith("dyn_edge.") for k in names) == bool(kw.get("include_dynedge"))


def test_default_parameter_count():
    """The default configuration (hidden 384, 12 + 4 blocks, seq_length 192), counted from the restatement."""
    import graphnet_amd as g
    count = sum(p.numel() for p in ref.DeepIce().parameters())
    assert count == 30_170_976
    assert sum(p.numel() for p in g.DeepIce().parameters()) == count
    assert g.DeepIce().no_weight_decay() == {"cls_token"}


def test_too_few_features_and_bad_widths_raise():
    import graphnet_amd as g
    with pytest.raises(ValueError, match="x, y, z and time"):
        g.DeepIce(n_features=3, **SMALL)
    with pytest.raises(ValueError, match="multiple of head_size"):
        g.DeepIce(hidden_dim=80, head_size=32)
    with pytest.raises(NotImplementedError, match="dropout"):
        g.Block_rel(64, 2, attn_drop=0.1)
    with pytest.raises(NotImplementedError, match="never materialised"):
        g.SpacetimeEncoder(32)(torch.zeros(1, 3, 4))


def test_cpu_batch_is_refused():
    import graphnet_amd as g
    m = g.DeepIce(**SMALL)
    b = g.Batch(x=torch.zeros(5, 6), batch=torch.zeros(5, dtype=torch.int64), ptr=torch.tensor([0, 5]))
    with pytest.raises(RuntimeError, match="MI355X"):
        m(b)


_B_D32_STYLE_CONFIG = """
arguments:
  backbone:
    ModelConfig:
      arguments: {depth: 12, depth_rel: 4, dynedge_args: null, head_size: 32, hidden_dim: 768,
        include_dynedge: false, n_features: 6, n_rel: 1, scaled_emb: false, seq_length: 192}
      class_name: DeepIce
  gnn: null
  graph_definition:
    ModelConfig:
      arguments:
        columns: [0, 1, 2, 3]
        detector:
          ModelConfig:
            arguments: {}
            class_name: IceCubeKaggle
        dtype: torch.float32
        input_feature_names: [x, y, z, time, charge, auxiliary]
        nb_nearest_neighbours: 6
        node_definition:
          ModelConfig:
            arguments: {}
            class_name: NodesAsPulses
      class_name: KNNGraph
  optimizer_class: '!class torch.optim.adamw AdamW'
  optimizer_kwargs: {eps: 1e-07, lr: 1e-05, weight_decay: 0.05}
  scheduler_class: null
  scheduler_config: null
  scheduler_kwargs: null
  tasks:
  - ModelConfig:
      arguments:
        hidden_size: 768
        loss_function:
          ModelConfig:
            arguments: {}
            class_name: VonMisesFisher3DLoss
        target_labels: direction
      class_name: DirectionReconstructionWithKappa
class_name: StandardModel
"""


def test_b_d32_style_model_config_round_trips(tmp_path):
    """A ``StandardModel`` config in the layout of the reference's pretrained ``B_d32`` one, with its backbone block (the
    node definition is ``NodesAsPulses``: ``IceMixNodes`` is not part of this package)."""
    import graphnet_amd as g
    from graphnet_amd.model import ModelConfig
    path = tmp_path / "b_d32.yml"
    path.write_text(_B_D32_STYLE_CONFIG)
    m = g.Model.from_config(str(path))
    assert type(m) is g.StandardModel and type(m.backbone) is g.DeepIce
    bb = m.backbone
    assert bb.nb_outputs == 768 and len(bb.blocks) == 12 and len(bb.sandwich) == 4 and bb.n_rel == 1
    assert bb.sandwich[0].attn.num_heads == 24 and bb.rel_pos.projection.weight.shape == (32, 32)
    assert type(m._graph_definition._detector) is g.IceCubeKaggle
    assert m._optimizer_class is torch.optim.AdamW
    assert type(m._tasks[0]) is g.DirectionReconstructionWithKappa and type(m._tasks[0]._loss_function) is g.VonMisesFisher3DLoss
    text = m.config.dump()
    assert "DeepIce" in text and "IceCubeKaggle" in text
    again = (tmp_path / "again.yml")
    again.write_text(text)
    m2 = ModelConfig.load(str(again)).construct()
    assert m2.config.dump() == text
    assert list(m2.state_dict()) == list(m.state_dict())
    alone = g.Model.from_config(bb.config)
    assert _shapes(alone) == _shapes(bb)


def test_icecube_kaggle_standardises_to_the_closed_form():
    import graphnet_amd as g
    det = g.IceCubeKaggle()
    names = ["x", "y", "z", "time", "charge", "auxiliary"]
    raw = np.array([[250.0, -125.0, 500.0, 1.0e4, 1000.0, 1.0],
                    [-500.0, 50.0, -250.0, 2.5e4, 1.0, 0.0],
                    [0.0, 10.0, 5.0, 4.0e4, 10.0, 1.0]], dtype=np.float32)
    out = det(torch.from_numpy(raw.copy()), names)
    want = raw.copy()
    want[:, :3] = raw[:, :3] / np.float32(500.0)
    want[:, 3] = (raw[:, 3] - np.float32(1.0e4)) / np.float32(3.0e4)
    assert np.array_equal(out.numpy()[:, [0, 1, 2, 3, 5]], want[:, [0, 1, 2, 3, 5]])
    # log10(charge) / 3 of 1000, 1, 10; an fp32 log10 may be one ulp off (2.4e-7 at 3)
    assert np.allclose(out.numpy()[:, 4].astype(np.float64), [1.0, 0.0, 1.0 / 3.0], rtol=0, atol=2e-7)
    assert out.numpy()[0, [0, 1, 2, 3, 5]].tolist() == [0.5, -0.25, 1.0, 0.0, 1.0]
    assert det.sensor_position_names == ["x", "y", "z"] and det.string_index_name == "string" and det.sensor_index_name == "sensor_id"
    assert det.geometry_table_file == ("icecube", "icecube86.parquet")
    with pytest.raises(KeyError):
        det(torch.zeros(1, 1), ["dom_x"])


def _event(L, seed, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.cat([torch.rand(L, 3, generator=gen) * 2.4 - 1.2, torch.rand(L, 1, generator=gen) * 0.9 - 0.3], 1)
    x0[L // 2:, :3] = x0[L // 2 - 1, :3]                       # one DOM position for the second half: time-like pairs
    return x0


@pytest.mark.parametrize("L,H,dh", [(65, 3, 32), (7, 1, 32), (33, 2, 64)])
def test_dense_bias_equals_the_factored_form(L, H, dh):
    """``softmax(q~ k + q~ R) (v + R)`` with ``R = W s + b`` materialised equals ``O + U W^T + b`` from the scores
    ``q~ k + (W^T q~) s``: forward and the five gradients, float64, 1e-12."""
    x0 = _event(L, 3)
    gen = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(L, H * dh, generator=gen, dtype=torch.float64) for _ in range(3))
    W = torch.randn(dh, dh, generator=gen, dtype=torch.float64) / dh ** 0.5
    b = torch.randn(dh, generator=gen, dtype=torch.float64) * 0.1
    s = ref.sin_emb(ref.pair_argument(x0).double(), dh)
    assert (ref.pair_argument(x0) < 0).any() and (ref.pair_argument(x0) > 0).any()
    pa = [t.clone().requires_grad_() for t in (q, k, v, W, b)]
    pb = [t.clone().requires_grad_() for t in (q, k, v, W, b)]
    dense = ref.dense_rel_attention(pa[0], pa[1], pa[2], s @ pa[3].t() + pa[4], H)
    fact = ref.factored_rel_attention(pb[0], pb[1], pb[2], s, pb[3], pb[4], H)
    gout = torch.randn(dense.shape, generator=gen, dtype=torch.float64)
    dense.backward(gout)
    fact.backward(gout)
    err = lambda a, r: float((a - r).abs().max() / r.abs().max())
    assert err(fact.detach(), dense.detach()) < 1e-12
    for x, y in zip(pb, pa):
        assert err(x.grad, y.grad) < 1e-12


def test_pair_argument_takes_the_correctly_rounded_square_root():
    """Every operation of the contract against numpy's fp32 arithmetic (IEEE, correctly rounded, ``np.sqrt`` included) on
    2016 pairs: ``torch.sqrt`` on a CPU fp32 tensor is an ulp off on some of them, which is 4.9e-4 rad at ``d`` near 4."""
    x0 = _event(64, 11).to(torch.float32)
    x = x0.numpy()
    d = x[:, None, :4] - x[None, :, :4]
    ds = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) - (d[..., 3] * np.float32(18.0)) ** 2
    assert ds.dtype == np.float32
    want = np.float32(1024.0) * np.clip(np.sign(ds) * np.sqrt(np.abs(ds)), np.float32(-4.0), np.float32(4.0))
    assert np.array_equal(ref.pair_argument(x0).numpy(), want)
    assert np.array_equal(want, np.float32(1024.0) * np.clip(np.sign(ds) * np.sqrt(np.abs(ds).astype(np.float64)).astype(np.float32), -4, 4))


def test_pair_argument_contract():
    """fp32, one rounding per operation; the factor of the time difference is exactly 18; repeated positions give
    ``ds < 0`` off the diagonal and 0 on it; the clip at +-4 acts."""
    x0 = torch.tensor([[0.1, 0.2, 0.3, 0.00], [0.1, 0.2, 0.3, 0.01], [0.1, 0.2, 0.3, 0.90], [1.1, -0.9, 0.3, 0.00],
                       [-1.2, 1.2, -1.2, 0.0], [1.2, -1.2, 1.2, 0.0]])
    a = ref.pair_argument(x0)
    assert a.dtype == torch.float32 and torch.equal(a.diagonal(), torch.zeros(6))
    assert float(a[0, 1]) == -1024.0 * float(torch.tensor(0.01, dtype=torch.float32) * 18.0)
    assert float(a[0, 2]) == -4096.0 and float(a[4, 5]) == 4096.0
    assert torch.equal(a, a.t())
    x, y = np.float32(1.1) - np.float32(0.1), np.float32(-0.9) - np.float32(0.2)
    assert float(a[3, 0]) == float(np.float32(1024.0) * np.sqrt(np.float32(x * x) + np.float32(y * y), dtype=np.float32))
