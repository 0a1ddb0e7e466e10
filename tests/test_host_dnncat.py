"""CPU: the DNNCat backbone's host side -- parameter layout against the reference's recorded state_dict, what it refuses,
which diffusion modes accept it, and the argument checks of csrc/cat.hip's C entry points (their declaration, export and
binding: tests/test_host_abi.py; cat.hip in the build lists: test_build_lists_name_every_source_and_header)."""
import pytest
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from tests import helpers as H

TRAIN_CASES = ["tiny_x0", "ragged_eps_wd", "deep_x0", "wide_x0"]


def _model(I=64, dims=(16,), **kw):
    dims = list(dims)
    return gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], 10, **kw)


def _diffusion(cat=True):
    return gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu", CatOneHot=cat)


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_parameters_match_the_reference_state_dict(case):
    fx = H.load("dnncat_train_" + case)
    meta = H.onehot_train_meta(fx)
    sd = H.state_dict_from(fx)
    m = _model(meta["I"], meta["dims"])
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sd.items()]
    assert [k for k, _ in m.named_parameters()][:4] == ["emb_layer.weight", "emb_layer.bias", "cat_layer.weight", "cat_layer.bias"]
    assert m.cat_layer.weight.shape == (1, 3) and m.cat_layer.bias.shape == (1,)
    m.load_state_dict(sd)
    assert all(torch.equal(m.state_dict()[k], sd[k]) for k in sd)
    assert [id(w) for w, _, _ in m.layer_list()] == [id(l.weight) for l in list(m.in_layers) + list(m.out_layers)]


def test_refusals():
    with pytest.raises(NotImplementedError, match="norm"):
        _model(norm=True)
    for dt in ("bf16", "f32x3"):
        with pytest.raises(NotImplementedError, match="f32"):
            _model(gemm_dtype=dt)
    m = _model()
    opt = gdmcf_amd.FusedAdamW(m.parameters(), lr=1e-3)
    with pytest.raises(NotImplementedError, match="first layer"):
        opt.fuse_into_backward(m)
    with pytest.raises(NotImplementedError, match="first layer"):
        opt.fuse_into_backward(m, min_numel=1)
    assert m.engine.fused_opt is None and all(p.is_contiguous() for p in m.parameters())
    assert opt.unfuse(m) is opt  # (nothing was fused: nothing to refuse)
    from gdmcf_amd.graph import GraphedTrainStep
    for diff in (_diffusion(True), _diffusion(False)):
        with pytest.raises(NotImplementedError):
            GraphedTrainStep(diff, m, opt, None, 8)
    assert not m.engine.supports_grad_sink and m.csr_rows is False


def test_onehot_model_accepts_dnncat_without_indexin_only():
    m, d = _model(), _diffusion()
    assert d._onehot_model(m) is m
    d.indexIn = True
    with pytest.raises(NotImplementedError):
        d._onehot_model(m)
    d.indexIn = False
    with pytest.raises(TypeError):
        d._onehot_model(gdmcf_amd.DNN([64, 16], [16, 64], 10))
    assert not isinstance(m, gdmcf_amd.DNN)  # (the continuous diffusion and the graphed step still want the plain DNN)


def test_cat_entry_points_check_their_arguments():
    lib = _lib.load()
    assert lib.gdmcf_cat_grad_ws_bytes(3, 4100) == 3 * 2 * 16 and lib.gdmcf_cat_grad_ws_bytes(1, 5) == 16
    assert lib.gdmcf_cat_grad_ws_bytes(0, 5) == 0
    # an empty batch, then null pointers: refused before anything is launched
    assert lib.gdmcf_cat_prep_input_f32(None, 8, None, 16, None, None, None, 0, None, 0, 0, None, 0, 0.5, 0, 0, None, None, None,
                                        None, 10, 0, 8, None, 64, None, 64, None, None) == _lib.E_SHAPE
    assert lib.gdmcf_cat_prep_input_f32(None, 8, None, 16, None, None, None, 0, None, 0, 0, None, 0, 0.5, 0, 0, None, None, None,
                                        None, 10, 2, 8, None, 64, None, 64, None, None) == _lib.E_ARG
    assert lib.gdmcf_cat_grad_f32(None, 8, None, 8, None, 16, 0, None, 0, 0.5, 0, 0, 2, 8, None, 0, None, None, None) == _lib.E_ARG
    assert lib.gdmcf_cat_grad_f32(None, 4, None, 8, None, 16, 0, None, 0, 0.5, 0, 0, 2, 8, None, 0, None, None, None) == _lib.E_SHAPE


def test_dnncat_has_no_cpu_fallback():
    m = _model().eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.zeros(2, 64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 64, 2))
    with pytest.raises(RuntimeError, match="MI355X"):
        _diffusion().training_losses(m, torch.zeros(2, 64), True)
