"""CPU: the host side of gdmcf_amd.recommend -- gdmcf_topk_masked_rows_f32 is declared, exported and bound and
refuses bad arguments before any launch with a message that names it; the new keywords and their defaults; the truth table of
the route (recommend.route_of) on objects that need no GPU, with the two predicates of p_sample answering what they answered
before; a CPU DeviceCSR is refused the way p_sample refuses a CPU tensor."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import route_of

ENTRY = "gdmcf_topk_masked_rows_f32"


def _call(lib, pred=4096, ldp=64, B=2, I=64, ip=4096, ix=4096, ip2=None, ix2=None, rows=4096, scale=None, k=5, idx=4096, val=None):
    return lib.gdmcf_topk_masked_rows_f32(pred, ldp, B, I, ip, ix, ip2, ix2, rows, scale, k, idx, val, None)


def test_entry_point_is_declared_exported_and_bound():
    assert ENTRY in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    fn = getattr(lib, ENTRY)
    assert len(fn.argtypes) == 14 and fn.restype is _lib.c_int
    with open(_lib.HEADER_PATH) as fh:
        assert ENTRY in fh.read()
    assert "recommend" in gdmcf_amd.__all__ and callable(gdmcf_amd.recommend)


def test_entry_point_refuses_bad_arguments_by_name():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory);
    every refusal leaves a message that names the entry."""
    lib = _lib.load()

    def refused(code, **kw):
        assert _call(lib, **kw) == code, kw
        assert ENTRY.encode() in lib.gdmcf_last_error(), (kw, lib.gdmcf_last_error())

    refused(_lib.E_SHAPE, k=0)
    refused(_lib.E_SHAPE, k=65)                       # k > I
    refused(_lib.E_ARG, k=2049, I=4096, ldp=4096)     # beyond the selection's limit
    refused(_lib.E_ARG, ix=None)                      # one of indptr / indices missing
    refused(_lib.E_ARG, ip=None)
    refused(_lib.E_ARG, ip2=4096)                     # ... of the second CSR
    refused(_lib.E_ARG, ix2=4096)
    refused(_lib.E_ARG, ip=None, ix=None, ip2=4096, ix2=4096)  # a second CSR without the first
    refused(_lib.E_SHAPE, B=0)
    refused(_lib.E_SHAPE, B=-3)
    refused(_lib.E_SHAPE, ldp=63)
    refused(_lib.E_SHAPE, I=0, ldp=0)


def test_keyword_defaults():
    assert inspect.signature(driver.evaluate).parameters["recommend"].default is False
    sig = inspect.signature(gdmcf_amd.recommend).parameters
    assert sig["mask"].default == "rows" and sig["sampling_steps"].default == 0 and sig["batch_size"].default == 400
    assert sig["sampling_noise"].default is False and sig["return_values"].default is False
    for name in ("mask", "sampling_steps", "sampling_noise", "batch_size", "return_values"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY
    from gdmcf_amd.engine import DenoiserEngine
    from gdmcf_amd.onehot import OneHotEngine
    assert inspect.signature(DenoiserEngine.p_sample_loop).parameters["stop"].default is False
    assert inspect.signature(DenoiserEngine._latent_loop).parameters["stop"].default is False
    assert inspect.signature(OneHotEngine.latent_loop).parameters["stop"].default is False


def _diff(mean_type=ModelMeanType.START_X, scale=0.01, schedule="linear-var"):
    return gdmcf_amd.GaussianDiffusion(mean_type, schedule, scale, 0.001, 0.01, 5, "cpu")


def _csr(I, values=None):
    m = sp.csr_matrix((np.random.default_rng(0).random((6, I)) < 0.2).astype(np.float64))
    if values is not None:
        m.data[:] = values
    return DeviceCSR(m, "cpu")


def test_route_truth_table():
    I = 64
    rows, weighted = _csr(I), _csr(I, 2.0)
    assert rows.values is None and weighted.values is not None
    ok = _diff()
    dnn = gdmcf_amd.DNN([I, 16], [16, I], 10).eval()
    assert route_of(ok, dnn, rows) == "latent-csr" and route_of(ok, dnn, rows, 0, False) == "latent-csr"
    for schedule in ("linear", "cosine", "binomial"):
        assert route_of(_diff(schedule=schedule), dnn, rows) == "latent-csr"
    # the rows must be dense: sampling steps, values other than 1
    assert route_of(ok, dnn, rows, 3) == "latent"
    assert route_of(ok, dnn, weighted) == "latent"
    # everything the latent loop does not cover
    assert route_of(_diff(mean_type=ModelMeanType.EPSILON), dnn, rows) == "item"
    assert route_of(_diff(scale=0.0), dnn, rows) == "item"
    assert route_of(ok, dnn, rows, 0, True) == "item"
    assert route_of(ok, gdmcf_amd.DNN([I, 16], [16, I], 10, norm=True).eval(), rows) == "item"
    training = gdmcf_amd.DNN([I, 16], [16, I], 10).train()
    assert route_of(ok, training, rows) == "item"
    training.drop.p = 0.0
    assert route_of(ok, training, rows) == "latent-csr"
    for dt in ("bf16", "f32x3"):
        assert route_of(ok, gdmcf_amd.DNN([I, 16], [16, I], 10, gemm_dtype=dt).eval(), rows) == "item"
    assert route_of(ok, gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval(), rows) == "item"
    # a table set whose c1[0] is not positive: checked on the host's table, once per table set
    calls = []
    real = _lib.schedule_tables

    def spy(*a):
        calls.append(a)
        tabs = real(*a)
        tabs[_lib.TABLE_NAMES.index("posterior_mean_coef1")][0] = 0.0
        return tabs

    bad = _diff()
    try:
        _lib.schedule_tables = spy
        assert route_of(bad, dnn, rows) == "item" and route_of(bad, dnn, rows) == "item"
    finally:
        _lib.schedule_tables = real
    assert len(calls) == 1
    # the one-hot backbones, the GCN backbone included
    dd = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu", CatOneHot=True)
    gcn = gdmcf_amd.DNNOneHotEmbeddingGCN([I, 16], [16, I], 10, item_num=I, user_num=9).eval()
    for m in (gdmcf_amd.DNNOneHot([I, 16], [16, I], 10).eval(),
              gdmcf_amd.DNNOneHotEmbedding([I, 16], [16, I], 10, item_num=I, user_num=9).eval(), gcn):
        assert route_of(dd, m, rows) == "latent-csr" and route_of(dd, m, rows, 5) == "latent"
    assert route_of(dd, gdmcf_amd.DNNCat([I, 16], [16, I], 10).eval(), rows) == "item"
    # p_sample's own predicates answer what tests/test_host_latent.py pins: the GCN backbone has the latent loop and is still no
    # backbone of the sparse item-space loop
    batch = rows.batch(torch.arange(3))
    assert dd._latent_reverse_ok(gcn) and not dd._sparse_reverse_ok(gcn, batch, 0)
    assert ok._sparse_reverse_ok(dnn, batch, 0) and not ok._sparse_reverse_ok(dnn, batch, 1)
    assert not ok._latent_reverse_ok(dnn, True, None) and not ok._latent_reverse_ok(dnn, False, {})


def test_recommend_refuses_a_cpu_csr_like_p_sample_refuses_a_cpu_tensor():
    dnn = gdmcf_amd.DNN([64, 16], [16, 64], 10).eval()
    with pytest.raises(RuntimeError, match="MI355X"):
        gdmcf_amd.recommend(_diff(), dnn, _csr(64), [0, 1], 5)
    with pytest.raises(TypeError, match="DeviceCSR"):
        gdmcf_amd.recommend(_diff(), dnn, torch.zeros(2, 64), [0, 1], 5)
