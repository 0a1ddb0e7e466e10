"""CPU: the host side of gdmcf_amd.rank_targets -- gdmcf_rank_targets_f32 and gdmcf_rank_metrics_f64 are declared,
exported and bound and refuse bad arguments before any launch with a message that names them; evaluate_utils.rank_metrics against
computeTopNAccuracy on lists cut from random full orders; the argument errors of rank_targets and driver.evaluate(ranks=True) that
are raised before the GPU is touched; DeviceCSR.max_row_len."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver, evaluate_utils
from gdmcf_amd.data_utils import DeviceCSR

ENTRIES = {"gdmcf_rank_targets_f32": 16, "gdmcf_rank_metrics_f64": 8}


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    with open(_lib.HEADER_PATH) as fh:
        header = fh.read()
    for name, n_args in ENTRIES.items():
        assert name in _lib.EXPORTED_SYMBOLS and name in header
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args and fn.restype is _lib.c_int
    assert "rank_targets" in gdmcf_amd.__all__ and callable(gdmcf_amd.rank_targets)


def _rank(lib, pred=4096, ldp=64, B=2, I=64, ip=4096, ix=4096, ip2=None, ix2=None, tip=4096, tix=4096, rows=4096, G=3, out=4096,
          ldr=3, live=None):
    return lib.gdmcf_rank_targets_f32(pred, ldp, B, I, ip, ix, ip2, ix2, tip, tix, rows, G, out, ldr, live, None)


def test_rank_targets_entry_refuses_bad_arguments_by_name():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory)."""
    lib = _lib.load()

    def refused(code, **kw):
        assert _rank(lib, **kw) == code, kw
        assert b"gdmcf_rank_targets_f32" in lib.gdmcf_last_error(), (kw, lib.gdmcf_last_error())

    refused(_lib.E_SHAPE, B=0)
    refused(_lib.E_SHAPE, B=-3)
    refused(_lib.E_SHAPE, ldp=63)
    refused(_lib.E_SHAPE, I=0, ldp=0)
    refused(_lib.E_SHAPE, G=0)
    refused(_lib.E_SHAPE, G=4)                        # ldr < G
    refused(_lib.E_ARG, ix=None)                      # one of indptr / indices missing
    refused(_lib.E_ARG, ip=None)
    refused(_lib.E_ARG, ip2=4096)                     # ... of the second CSR
    refused(_lib.E_ARG, ix2=4096)
    refused(_lib.E_ARG, ip=None, ix=None, ip2=4096, ix2=4096)  # a second CSR without the first
    refused(_lib.E_ARG, tip=None)                     # the targets are required
    refused(_lib.E_ARG, tix=None)
    refused(_lib.E_ARG, out=None)
    refused(_lib.E_ARG, pred=None)
    # a row wider than the LDS plan takes (the mask bitmap alone exceeds a CU's 160 KiB)
    refused(_lib.E_UNSUPPORTED, I=1_400_000, ldp=1_400_000)


def test_rank_metrics_entry_refuses_bad_arguments_by_name():
    import ctypes
    lib = _lib.load()

    def call(ranks=4096, ldr=4, U=3, G=4, topN=(1, 5), out=4096):
        return lib.gdmcf_rank_metrics_f64(ranks, ldr, U, G, (ctypes.c_int * max(len(topN), 1))(*topN), len(topN), out, None)

    def refused(code, **kw):
        assert call(**kw) == code, kw
        assert b"gdmcf_rank_metrics_f64" in lib.gdmcf_last_error(), (kw, lib.gdmcf_last_error())

    refused(_lib.E_SHAPE, U=0)
    refused(_lib.E_SHAPE, G=0)
    refused(_lib.E_SHAPE, ldr=3)
    refused(_lib.E_SHAPE, topN=())
    refused(_lib.E_SHAPE, topN=tuple(range(1, 10)))   # nine cut-offs: the host calls in groups of eight
    refused(_lib.E_ARG, topN=(5, 5))
    refused(_lib.E_ARG, topN=(5, 1))
    refused(_lib.E_ARG, topN=(0, 1))
    refused(_lib.E_ARG, ranks=None)
    refused(_lib.E_ARG, out=None)


def _orders_and_truth(U, I, seed):
    rng = np.random.default_rng(seed)
    order = np.stack([rng.permutation(I) for _ in range(U)])
    truth = [sorted(rng.choice(I, size=int(n), replace=False).tolist()) for n in rng.integers(0, 26, U)]
    truth[0], truth[1] = [], [int(order[1, I - 1])]  # a user without ground truth; one whose only item sits last
    pos = np.argsort(order, axis=1)  # pos[u, item] = rank of the item
    G = max(max(len(t) for t in truth), 1)
    ranks = np.full((U, G), -1, dtype=np.int32)
    for u, t in enumerate(truth):
        ranks[u, :len(t)] = pos[u, t]
    return order, truth, ranks


def test_rank_metrics_equals_computeTopNAccuracy_on_the_lists_the_ranks_came_from():
    U, I = 40, 300
    order, truth, ranks = _orders_and_truth(U, I, 7)
    assert any(len(t) == 0 for t in truth) and any(len(t) > 20 for t in truth)
    topN = [1, 5, 20, 100, 300]  # N above the number of hits of every user; N == I
    want = evaluate_utils.computeTopNAccuracy(truth, order.tolist(), topN)
    got = evaluate_utils.rank_metrics(ranks, topN)
    assert got == want, (got, want)
    assert want[1][-1] > 0  # (the comparison is not one of zeros)
    # shuffled columns, and -1 between the entries: only the set of ranks per user matters
    rng = np.random.default_rng(1)
    wide = np.concatenate([ranks, np.full((U, 3), -1, dtype=np.int32)], axis=1)
    wide = np.stack([row[rng.permutation(len(row))] for row in wide])
    assert evaluate_utils.rank_metrics(wide, topN) == want
    # a cut-off above the item count counts every hit: recall is the share of users with ground truth
    above = evaluate_utils.rank_metrics(ranks, [1000])
    assert above[1] == [round(sum(1 for t in truth if t) / U, 4)]
    for bad in ([], [5, 5], [5, 1], [0, 3]):
        with pytest.raises(ValueError, match="topN"):
            evaluate_utils.rank_metrics(ranks, bad)


def _diff():
    return gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, "cpu")


def _csr(U, I, seed=0):
    return DeviceCSR(sp.csr_matrix((np.random.default_rng(seed).random((U, I)) < 0.2).astype(np.float64)), "cpu")


def test_max_row_len():
    m = sp.csr_matrix(np.array([[0, 1, 0, 1, 1], [0, 0, 0, 0, 0], [1, 0, 0, 0, 0]], dtype=np.float64))
    assert DeviceCSR(m, "cpu").max_row_len == 3
    assert DeviceCSR(sp.csr_matrix((4, 7)), "cpu").max_row_len == 0
    dup = sp.csr_matrix((np.ones(3), np.array([2, 2, 5]), np.array([0, 3])), shape=(1, 7))  # summed: two distinct items
    assert DeviceCSR(dup, "cpu").max_row_len == 2


def test_rank_targets_argument_errors_come_before_the_gpu():
    dnn = gdmcf_amd.DNN([64, 16], [16, 64], 10).eval()
    rows = _csr(6, 64)
    with pytest.raises(TypeError, match="rows must be"):
        gdmcf_amd.rank_targets(_diff(), dnn, torch.zeros(2, 64), [0, 1], rows)
    with pytest.raises(TypeError, match="targets must be"):
        gdmcf_amd.rank_targets(_diff(), dnn, rows, [0, 1], sp.csr_matrix((6, 64)))
    with pytest.raises(ValueError, match="shape"):
        gdmcf_amd.rank_targets(_diff(), dnn, rows, [0, 1], _csr(6, 65))
    with pytest.raises(ValueError, match="shape"):
        gdmcf_amd.rank_targets(_diff(), dnn, rows, [0, 1], _csr(5, 64))
    with pytest.raises(RuntimeError, match="MI355X"):  # a CPU DeviceCSR, as recommend refuses it
        gdmcf_amd.rank_targets(_diff(), dnn, rows, [0, 1], _csr(6, 64, 1))
    sig = inspect.signature(gdmcf_amd.rank_targets).parameters
    assert sig["mask"].default == "rows" and sig["sampling_steps"].default == 0 and sig["batch_size"].default == 400
    assert sig["sampling_noise"].default is False and sig["latent"].default is True and sig["return_live"].default is False
    for name in ("mask", "sampling_steps", "sampling_noise", "batch_size", "latent", "noise0", "sampled0", "return_live"):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY


def test_evaluate_ranks_needs_recommend_and_takes_no_candidates():
    assert inspect.signature(driver.evaluate).parameters["ranks"].default is False
    m = sp.csr_matrix((np.random.default_rng(0).random((6, 64)) < 0.2).astype(np.float64))
    dnn = gdmcf_amd.DNN([64, 16], [16, 64], 10).eval()
    with pytest.raises(ValueError, match="ranks"):
        driver.evaluate(_diff(), dnn, m, m, m, [5], 0, False, 4, "cpu", ranks=True)
    with pytest.raises(ValueError, match="ranks"):
        driver.evaluate(_diff(), dnn, m, m, m, [5], 0, False, 4, "cpu", recommend=True, ranks=True, candidates=np.zeros((6, 8), dtype=np.int64))
