"""CPU: the host side of candidate lists -- gdmcf_cand_scores_f32 and gdmcf_cand_pick_f32 are declared, exported and
bound and refuse bad arguments before any launch; the route rule on a grid; the argument errors of recommend(candidates=) and
score_candidates, raised before anything touches a device; the new keywords and their defaults."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import candidate_route_of

ENTRIES = {"gdmcf_cand_scores_f32": 20, "gdmcf_cand_pick_f32": 16}


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as fh:
        header = fh.read()
    for name, n_args in ENTRIES.items():
        assert name in _lib.EXPORTED_SYMBOLS and name in header
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args and fn.restype is _lib.c_int
    for name in ("recommend", "score_candidates"):
        assert name in gdmcf_amd.__all__ and callable(getattr(gdmcf_amd, name))


def _scores(lib, A=4096, lda=64, W=4096, ldw=64, I=50, K=64, bias=None, scale=None, cand=4096, ldcand=8, B=2, C=8, ip=None, ix=None,
            ip2=None, ix2=None, rows=None, out=4096, ldo=8):
    return lib.gdmcf_cand_scores_f32(A, lda, W, ldw, I, K, bias, scale, cand, ldcand, B, C, ip, ix, ip2, ix2, rows, out, ldo, None)


def _pick(lib, dense=4096, ldd=64, B=2, I=50, scale=None, cand=4096, ldcand=8, C=8, ip=None, ix=None, ip2=None, ix2=None, rows=None,
          out=4096, ldo=8):
    return lib.gdmcf_cand_pick_f32(dense, ldd, B, I, scale, cand, ldcand, C, ip, ix, ip2, ix2, rows, out, ldo, None)


def test_entry_points_refuse_bad_arguments_by_name():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory);
    every refusal leaves a message that names the entry."""
    lib = _lib.load()
    for call, name in ((_scores, "gdmcf_cand_scores_f32"), (_pick, "gdmcf_cand_pick_f32")):
        def refused(code, **kw):
            assert call(lib, **kw) == code, (name, kw)
            assert name.encode() in lib.gdmcf_last_error(), (kw, lib.gdmcf_last_error())

        refused(_lib.E_SHAPE, B=0)
        refused(_lib.E_SHAPE, B=-3)
        refused(_lib.E_SHAPE, C=0)
        refused(_lib.E_SHAPE, I=0)
        refused(_lib.E_SHAPE, ldo=7)
        refused(_lib.E_SHAPE, ldcand=7)                   # neither 0 (shared) nor >= C
        refused(_lib.E_ARG, ip=4096)                      # one of indptr / indices missing
        refused(_lib.E_ARG, ix=4096)
        refused(_lib.E_ARG, ip=4096, ix=4096, ip2=4096)   # ... of the second CSR
        refused(_lib.E_ARG, ip2=4096, ix2=4096)           # a second CSR without the first
        refused(_lib.E_ARG, cand=None)
        refused(_lib.E_ARG, out=None)
    for K in (0, -1, 4097):
        assert _scores(lib, K=K, lda=8192, ldw=8192) == _lib.E_SHAPE and b"gdmcf_cand_scores_f32" in lib.gdmcf_last_error()
    assert _scores(lib, lda=63) == _lib.E_SHAPE and _scores(lib, ldw=63) == _lib.E_SHAPE
    assert _scores(lib, A=None) == _lib.E_ARG and _scores(lib, W=None) == _lib.E_ARG
    assert _pick(lib, ldd=49) == _lib.E_SHAPE and _pick(lib, dense=None) == _lib.E_ARG


def test_route_rule_on_a_grid():
    for I in (1, 131, 38048):
        for B in (1, 2, 7, 16, 400):
            for C in (1, 20, 100, 500, 2000, I, I + 1):
                assert candidate_route_of(B, C, I, False) == "picked"
                assert candidate_route_of(B, C, I, True) == ("gathered" if B * C <= I else "picked"), (B, C, I)
    # the edge, and sizes whose product passes 2^31
    assert candidate_route_of(1, 131, 131, True) == "gathered" and candidate_route_of(1, 132, 131, True) == "picked"
    assert candidate_route_of(131, 1, 131, True) == "gathered" and candidate_route_of(2, 66, 131, True) == "picked"
    assert candidate_route_of(2 ** 20, 2 ** 20, 2 ** 31 - 1, True) == "picked"
    assert candidate_route_of(np.int64(2), torch.tensor(20), 131, True) == "gathered"


def _diff():
    return gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu")


def _csr(I):
    return DeviceCSR(sp.csr_matrix((np.random.default_rng(0).random((6, I)) < 0.2).astype(np.float64)), "cpu")


def test_argument_errors_come_before_any_device_work():
    """Every one is raised ahead of the check that the rows live on a GPU (which this machine would fail with RuntimeError)."""
    dnn = gdmcf_amd.DNN([64, 16], [16, 64], 10).eval()
    diff, rows, ids = _diff(), _csr(64), [0, 1, 2]
    ok = torch.arange(12).reshape(3, 4)
    with pytest.raises(AssertionError, match="k out of range"):
        gdmcf_amd.recommend(diff, dnn, rows, ids, 5, candidates=ok)                       # k > C
    with pytest.raises(AssertionError, match="k out of range"):
        gdmcf_amd.recommend(diff, dnn, rows, ids, 0, candidates=ok)
    for call in (lambda **kw: gdmcf_amd.recommend(diff, dnn, rows, ids, 2, **kw),
                 lambda **kw: gdmcf_amd.score_candidates(diff, dnn, rows, ids, kw.pop("candidates"), **kw)):
        with pytest.raises(ValueError, match="rows for 3 user ids"):
            call(candidates=torch.arange(8).reshape(2, 4))                                # the wrong number of rows
        with pytest.raises(ValueError, match=r"\[n, C\]"):
            call(candidates=torch.zeros(3, 2, 2, dtype=torch.int64))                      # 3-D
        with pytest.raises(ValueError, match="no item"):
            call(candidates=torch.zeros(3, 0, dtype=torch.int64))
        with pytest.raises(TypeError, match="integers"):
            call(candidates=torch.zeros(3, 4))
        with pytest.raises(ValueError, match="candidate_route"):
            call(candidates=ok, candidate_route="fastest")
        with pytest.raises(RuntimeError, match="MI355X"):                                 # well-formed: on to the device check
            call(candidates=ok)
        with pytest.raises(RuntimeError, match="MI355X"):
            call(candidates=[5, 1, -1, 2 ** 40])                                          # a shared list, as a sequence
    with pytest.raises(TypeError, match="DeviceCSR"):
        gdmcf_amd.score_candidates(diff, dnn, torch.zeros(3, 64), ids, ok)
    with pytest.raises(ValueError, match="recommend=True"):
        driver.evaluate(diff, dnn, sp.csr_matrix((3, 64)), sp.csr_matrix((3, 64)), sp.csr_matrix((3, 64)), [5], 0, False, 2, "cpu",
                        candidates=ok)


def test_keyword_defaults_leave_every_call_as_it_was():
    sig = inspect.signature(gdmcf_amd.recommend).parameters
    assert sig["candidates"].default is None and sig["candidate_route"].default == "auto"
    assert sig["candidates"].kind is inspect.Parameter.KEYWORD_ONLY and sig["candidate_route"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(driver.evaluate).parameters["candidates"].default is None
    sig = inspect.signature(gdmcf_amd.score_candidates).parameters
    assert list(sig)[:5] == ["diffusion", "model", "rows", "user_ids", "candidates"]
    want = dict(mask="rows", sampling_steps=0, sampling_noise=False, batch_size=400, latent=True, candidate_route="auto")
    for name, default in want.items():
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
