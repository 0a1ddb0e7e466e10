"""CPU: the host side of the reverse loop in the first hidden layer's space -- gdmcf_latent_step_f32's refusals, the `latent`
keywords (all off by default) and the truth table of GaussianDiffusion._latent_reverse_ok, the one predicate that picks the route."""
import inspect

import pytest
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd import build as gbuild


def _call(lib, A=4096, M=4096, pc=4096, c1=4096, c2=4096, pn=4096, h=None, act=0, B=2, N=8, K=8, lda=8, ldm=8, ldpc=8, ldpn=8, ldh=8):
    return lib.gdmcf_latent_step_f32(A, lda, M, ldm, None, pc, ldpc, c1, c2, None, act, B, N, K, pn, ldpn, h, ldh, None, 0, None)


def test_latent_step_entry_point_checks_its_arguments():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory)."""
    lib = _lib.load()
    assert "gdmcf_latent_step_f32" in _lib.EXPORTED_SYMBOLS and "gdmcf_latent_step_ws_bytes" in _lib.EXPORTED_SYMBOLS
    assert lib.gdmcf_latent_step_ws_bytes(400, 1000, 1000) == 0
    for dim in ("B", "N", "K"):
        assert _call(lib, **{dim: 0}) == _lib.E_SHAPE
    assert _call(lib, B=0, A=None) == _lib.E_SHAPE  # ... before the null pointers
    for ptr in ("A", "M", "pc", "c1", "c2", "pn"):
        assert _call(lib, **{ptr: None}) == _lib.E_ARG
    assert _call(lib, act=2) == _lib.E_ARG
    for ld in ("lda", "ldm", "ldpc", "ldpn"):
        assert _call(lib, **{ld: 7}) == _lib.E_SHAPE
    assert _call(lib, h=4096, ldh=7) == _lib.E_SHAPE
    assert b"latent_step" in lib.gdmcf_last_error()


def test_latent_step_source_is_in_the_build_lists():
    assert "latent_step.hip" in gbuild.SOURCES and "latent_step.hip" in gbuild.NO_SPILL and "latent_step.hip" in gbuild.STORE_LINT


def test_the_latent_keywords_exist_and_default_to_off():
    for fn in (gdmcf_amd.GaussianDiffusion.p_sample, gdmcf_amd.GaussianDiffusionDiscrete.p_sample, driver.evaluate):
        assert inspect.signature(fn).parameters["latent"].default is False
    from gdmcf_amd.engine import DenoiserEngine
    assert inspect.signature(DenoiserEngine.p_sample_loop).parameters["latent"].default is False
    d = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu")
    assert d.last_reverse_route is None


def _diff(mean_type=ModelMeanType.START_X, scale=0.01, schedule="linear-var"):
    return gdmcf_amd.GaussianDiffusion(mean_type, schedule, scale, 0.001, 0.01, 5, "cpu")


def test_latent_reverse_ok_truth_table():
    I = 64
    dnn = gdmcf_amd.DNN([I, 16], [16, I], 10).eval()
    ok = _diff()
    assert ok._latent_reverse_ok(dnn) and ok._latent_reverse_ok(dnn, False, None)
    for schedule in ("linear", "cosine", "binomial"):  # posterior_mean_coef2[0] is exactly 0 for every schedule
        d = _diff(schedule=schedule)
        assert float(d._t32["c2"][0]) == 0.0 and d._latent_reverse_ok(dnn)
    deep = gdmcf_amd.DNN([I, 24, 16], [16, 24, I], 10).eval()
    assert ok._latent_reverse_ok(deep)
    # one condition off at a time
    assert not _diff(mean_type=ModelMeanType.EPSILON)._latent_reverse_ok(dnn)
    assert not _diff(scale=0.0)._latent_reverse_ok(dnn)
    assert not ok._latent_reverse_ok(dnn, True, None)          # sampling noise
    assert not ok._latent_reverse_ok(dnn, False, {})           # capture, even an empty dict
    assert not ok._latent_reverse_ok(gdmcf_amd.DNN([I, 16], [16, I], 10, norm=True).eval())
    training = gdmcf_amd.DNN([I, 16], [16, I], 10).train()
    assert not ok._latent_reverse_ok(training)                 # active dropout
    training.drop.p = 0.0
    assert ok._latent_reverse_ok(training)                     # ... a training-mode model without dropout is fine
    for dt in ("bf16", "f32x3"):
        assert not ok._latent_reverse_ok(gdmcf_amd.DNN([I, 16], [16, I], 10, gemm_dtype=dt).eval())
    # the tables: a last step that still needs x_1, a non-finite c1
    bad = _diff()
    bad._t32 = dict(bad._t32, c2=bad._t32["c2"].clone())
    bad._t32["c2"][0] = 1e-3
    assert not bad._latent_reverse_ok(dnn)
    bad = _diff()
    bad._t32 = dict(bad._t32, c1=bad._t32["c1"].clone())
    bad._t32["c1"][2] = float("inf")
    assert not bad._latent_reverse_ok(dnn)
    # exact types: the four backbones whose engines have the loop; a subclass (DNNCat is one) takes the item-space route
    class Sub(gdmcf_amd.DNN):
        pass
    assert not ok._latent_reverse_ok(Sub([I, 16], [16, I], 10).eval())
    assert not ok._latent_reverse_ok(gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval())
    dd = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu", CatOneHot=True)
    assert dd._latent_reverse_ok(gdmcf_amd.DNNOneHot([I, 16], [16, I], 10).eval())
    assert dd._latent_reverse_ok(gdmcf_amd.DNNOneHotEmbedding([I, 16], [16, I], 10, item_num=I, user_num=9).eval())
    assert dd._latent_reverse_ok(gdmcf_amd.DNNOneHotEmbeddingGCN([I, 16], [16, I], 10, item_num=I, user_num=9).eval())
    assert not dd._latent_reverse_ok(gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval())
    eps = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.EPSILON, "linear-var", 0.01, 0.001, 0.01, 5, "cpu", CatOneHot=True)
    assert not eps._latent_reverse_ok(gdmcf_amd.DNNOneHot([I, 16], [16, I], 10).eval())


def test_latent_p_sample_refuses_a_cpu_tensor_like_the_item_route():
    dnn = gdmcf_amd.DNN([64, 16], [16, 64], 10).eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        _diff().p_sample(dnn, torch.zeros(2, 64), 0, False, latent=True)
