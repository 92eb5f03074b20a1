"""CPU: ``ConvNet`` / ``TAGConv`` construct with the reference's state-dict layout, refuse what the kernels do not cover, and
the TAGConv entries reject bad arguments on the host before any launch (there is no GPU here)."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from graphnet_amd import _lib
    return _lib.lib()


def test_state_dict_layout_of_the_reference():
    from graphnet_amd import ConvNet, ModelConfig
    m = ConvNet(7, 3)
    want = {f"conv{l}.lins.{k}.weight": (128, 7 if l == 1 else 128) for l in (1, 2, 3) for k in range(3)}
    want.update({f"conv{l}.bias": (128,) for l in (1, 2, 3)})
    want.update({f"batchnorm1.{n}": (768,) for n in ("weight", "bias", "running_mean", "running_var")})
    want["batchnorm1.num_batches_tracked"] = ()
    for l in range(1, 6):
        want.update({f"linear{l}.weight": (768, 768), f"linear{l}.bias": (768,)})
    want.update({"out.weight": (3, 768), "out.bias": (3,)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert m.nb_inputs == 7 and m.nb_outputs == 3 and m.drop3.p == 0.3
    m2 = ModelConfig("ConvNet", {"nb_inputs": 7, "nb_outputs": 3, "nb_intermediate": 64, "dropout_ratio": 0.1}).construct()
    assert isinstance(m2, ConvNet) and m2.nb_intermediate2 == 384 and m2.drop1.p == 0.1


@pytest.mark.parametrize("make", [lambda g: g.ConvNet(7, 3, nb_intermediate=100), lambda g: g.TAGConv(32, 32, K=3),
                                  lambda g: g.TAGConv(32, 32, normalize=False), lambda g: g.ConvNet(7, 3, nb_intermediate=288)])
def test_shapes_outside_the_kernels_raise(make):
    import graphnet_amd
    with pytest.raises(NotImplementedError):
        make(graphnet_amd)


@pytest.mark.parametrize("C", [0, 48, 288])
def test_bad_widths_are_rejected_on_the_host(lib, C):
    p = 256                                                  # (never dereferenced: every call returns before the launch)
    assert lib.gn_tagconv_supported(C, 128) == 0 and lib.gn_tagconv_supported(128, C) == 0 and lib.gn_tagconv_supported(32, 256) == 1
    calls = {
        "gn_tag_propagate": lambda: lib.gn_tag_propagate(p, 512, p, p, p, 10, 8, C, p, 512, None),
        "gn_tag_propagate_t": lambda: lib.gn_tag_propagate_t(p, 512, p, 512, p, p, p, p, p, p, 10, 8, C, p, 512, None),
        "gn_tagconv_fwd": lambda: lib.gn_tagconv_fwd(0, p, 512, p, 512, p, p, p, 10, 8, C, p, p, 128, p, 512, p, 512, None),
    }
    for name, call in calls.items():
        assert call() != 0 and name.encode() in lib.gn_last_error() and b"C%32" in lib.gn_last_error()
    assert lib.gn_tagconv_fwd(0, p, 512, p, 512, p, p, p, 10, 8, 128, p, p, C, p, 512, p, 512, None) != 0
    assert lib.gn_tag_norm(p, p, 10, 33, p, None) != 0 and b"gn_tag_norm" in lib.gn_last_error()
    assert lib.gn_tag_dpre(p, 512, p, 512, 10, 6, p, 512, None) != 0 and b"gn_tag_dpre" in lib.gn_last_error()
