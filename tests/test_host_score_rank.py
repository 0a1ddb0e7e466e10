"""CPU (-m "not gpu"): the host side of the LightGCN rank surface -- gdmcf_score_rank_f32, gdmcf_score_rank_ws_bytes and
gdmcf_debug_score_rank_plan are declared, exported and bound and refuse bad arguments before any launch; the workspace does not
grow with the score matrix; evaluate_utils.score_rank, LightGCN.rank_targets and lightgcn.get_metrics_at refuse what they must
before the GPU is touched; get_metrics_at's hit matrix from ranks against one written by hand."""
import ctypes
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib
from gdmcf_amd.lightgcn import get_metrics_at, hits_from_ranks, ranking_terms
from tests.test_host_lightgcn_eval import _hand_case

P = ctypes.c_void_p
INT, I64, SZ = ctypes.c_int, ctypes.c_int64, ctypes.c_size_t


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    assert _lib._SIGNATURES["gdmcf_score_rank_ws_bytes"] == (SZ, [INT, INT, INT, INT])
    assert _lib._SIGNATURES["gdmcf_score_rank_f32"] == (INT, [P, I64, P, INT, P, I64, INT, INT, P, P, P, P, INT, P, I64, P, P, SZ, P])
    assert _lib._SIGNATURES["gdmcf_debug_score_rank_plan"] == (INT, [INT, INT, INT, P, P, P, P])
    for name in ("gdmcf_score_rank_ws_bytes", "gdmcf_score_rank_f32", "gdmcf_debug_score_rank_plan"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "score_rank" in gdmcf_amd.__all__ and callable(gdmcf_amd.score_rank)
    assert callable(gdmcf_amd.LightGCN.rank_targets)


def _call(lib, ue=4096, ldu=64, n_rows=8, ie=4096, ldi=64, n_items=100, d=64, ip=None, ix=None, tp=4096, tx=4096, G=3, out=4096,
          ldr=3, ws=4096, nb=1 << 30):
    return lib.gdmcf_score_rank_f32(ue, ldu, None, n_rows, ie, ldi, n_items, d, ip, ix, tp, tx, G, out, ldr, None, ws, nb, None)


def test_entry_refuses_bad_arguments_by_name():
    """Refused before anything is launched (the pointers are never read on the host: small integers stand in for device memory).
    The codes are gdmcf_score_topk_f32's and gdmcf_rank_targets_f32's for the same faults."""
    lib = _lib.load()

    def refused(code, **kw):
        assert _call(lib, **kw) == code, kw
        assert b"gdmcf_score_rank_f32" in lib.gdmcf_last_error(), (kw, lib.gdmcf_last_error())

    refused(_lib.E_SHAPE, n_rows=0)
    refused(_lib.E_SHAPE, n_items=0)
    refused(_lib.E_SHAPE, d=0)
    refused(_lib.E_SHAPE, ldu=63)
    refused(_lib.E_SHAPE, ldi=63)
    refused(_lib.E_SHAPE, G=0)
    refused(_lib.E_SHAPE, G=4)                      # ldr < G
    refused(_lib.E_ARG, d=4097, ldu=8192, ldi=8192)
    refused(_lib.E_ARG, ip=4096)                    # one of indptr / indices missing
    refused(_lib.E_ARG, ix=4096)
    refused(_lib.E_ARG, tp=None)                    # the targets are required
    refused(_lib.E_ARG, tx=None)
    refused(_lib.E_ARG, out=None)
    refused(_lib.E_ARG, ue=None)
    refused(_lib.E_ARG, ie=None)
    refused(_lib.E_WORKSPACE, ws=None)
    refused(_lib.E_WORKSPACE, nb=lib.gdmcf_score_rank_ws_bytes(8, 100, 64, 3) - 1)
    refused(_lib.E_ARG, ws=4100)                    # not 16-byte aligned


def _plan(lib, n_rows, n_items, G):
    v = [ctypes.c_int() for _ in range(4)]
    ok = lib.gdmcf_debug_score_rank_plan(n_rows, n_items, G, *[ctypes.byref(x) for x in v])
    return ok, tuple(x.value for x in v)


def test_plan_fits_the_lds_and_the_workspace_does_not_grow_with_the_score_matrix():
    lib = _lib.load()
    assert _plan(lib, 0, 10, 1) == (0, (0, 0, 0, 0)) and _plan(lib, 10, 10, 0) == (0, (0, 0, 0, 0))
    assert lib.gdmcf_score_rank_ws_bytes(0, 10, 64, 1) == 0 and lib.gdmcf_score_rank_ws_bytes(10, 10, 64, 0) == 0
    seen = set()
    for G in (1, 10, 16, 17, 128, 129, 256, 257, 512, 513, 1024, 1025, 5000):
        for n_rows, n_items in ((54574, 34395), (400, 34395), (40, 30000), (1, 1), (7, 100000)):
            ok, (R, GP, npass, nslab) = _plan(lib, n_rows, n_items, G)
            assert ok == 1 and R in (16, 32, 64) and GP & (GP - 1) == 0 and GP >= 16
            assert GP * npass >= G and (npass == 1 or GP * (npass - 1) < G)
            lds = 12 * R * GP + 4 * R + 4 * 64 * R + 8 * R  # pairs + counters, the below counter, the bitmap window, control words
            assert lds <= 160 * 1024
            seen.add(R)
            Gpad = -(-G // 16) * 16
            ws = lib.gdmcf_score_rank_ws_bytes(n_rows, n_items, 64, G)
            assert ws == n_rows * (8 * Gpad + 4 * npass * nslab * (GP + 1) + 4 * nslab)
            assert 1 <= nslab <= 16 and (nslab == 1 or 4 * nslab * (GP + 1) <= 0.05 * 4 * n_items)
            # the same for twice the items, up to the slab count: no term in n_rows * n_items
            ok2, (_, _, _, nslab2) = _plan(lib, n_rows, 2 * n_items, G)
            assert lib.gdmcf_score_rank_ws_bytes(n_rows, 2 * n_items, 64, G) == n_rows * (8 * Gpad + 4 * npass * nslab2 * (GP + 1) + 4 * nslab2)
    assert seen == {16, 32, 64}
    # all test users of the Yelp shape, ten targets each: 11 MB beside the 7.5 GB score matrix
    assert lib.gdmcf_score_rank_ws_bytes(54574, 34395, 64, 10) < 0.002 * 4 * 54574 * 34395


def test_python_functions_refuse_cpu_tensors_and_bad_shapes():
    ue, ie = torch.zeros(4, 8), torch.zeros(9, 8)
    tp, tx = torch.zeros(5, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        gdmcf_amd.score_rank(ue, ie, tp, tx)
    with pytest.raises(ValueError, match="required"):
        gdmcf_amd.score_rank(ue, ie, None, None)
    with pytest.raises(ValueError, match="go together"):
        gdmcf_amd.score_rank(ue, ie, tp, tx, mask_indptr=tp)
    sig = inspect.signature(gdmcf_amd.score_rank).parameters
    assert list(sig) == ["user_emb", "item_emb", "tgt_indptr", "tgt_indices", "mask_indptr", "mask_indices", "user_ids", "G",
                         "return_live", "check_ids"]
    assert sig["G"].default is None and sig["return_live"].default is False and sig["check_ids"].default is True
    assert "host read" in gdmcf_amd.score_rank.__doc__.lower()
    empty = sp.csr_matrix((4, 9))
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        get_metrics_at(ue, ie, 4, 9, empty, empty, [2])
    for bad in ([], [5, 5], [5, 1], [0, 3]):
        with pytest.raises(ValueError, match="ascending"):
            get_metrics_at(ue, ie, 4, 9, empty, empty, bad)


def test_lightgcn_rank_targets_argument_errors_come_before_the_gpu():
    U, I = 6, 9
    rows, cols = np.array([0, 1, 2, 3, 4, 5]), np.array([0, 1, 2, 3, 4, 5])
    lg = gdmcf_amd.LightGCN({"user_id_idx": rows, "item_id_idx": cols}, U, I, 1, 4, device="cpu")
    tgt = sp.csr_matrix((U, I))
    with pytest.raises(ValueError, match="required"):
        lg.rank_targets([0, 1], None)
    with pytest.raises(ValueError, match="shape"):
        lg.rank_targets([0, 1], sp.csr_matrix((U, I + 1)))
    with pytest.raises(ValueError, match="shape"):
        lg.rank_targets([0, 1], tgt, history=sp.csr_matrix((U - 1, I)))
    with pytest.raises(IndexError):
        lg.rank_targets([0, U], tgt)
    with pytest.raises(IndexError):
        lg.rank_targets([-1], tgt)
    sig = inspect.signature(gdmcf_amd.LightGCN.rank_targets).parameters
    assert list(sig) == ["self", "users", "targets", "history", "return_live"]
    assert sig["history"].default is None and sig["return_live"].default is False


def test_hit_matrix_from_ranks_reproduces_the_hand_worked_case():
    """The hand-worked case of tests/test_host_lightgcn_eval.py (K = 3) as ranks: user 0 has five test items, two of them at ranks
    0 and 2; user 1's only test item sits at rank 1; user 2's two test items sit past K."""
    _, gts, want = _hand_case()
    ranks = torch.tensor([[0, 2, 17, 5, 9], [1, -1, -1, -1, -1], [40, 3, -1, -1, -1]], dtype=torch.int32)
    hit = hits_from_ranks(ranks, 3)
    by_hand = torch.tensor([[True, False, True], [False, True, False], [False, False, False]])
    assert hit.dtype == torch.bool and torch.equal(hit, by_hand)
    n_gt = torch.tensor([len(g) for g in gts])
    got = tuple(float(t.mean()) for t in ranking_terms(hit, n_gt))
    assert got == tuple(float(t.mean()) for t in ranking_terms(by_hand, n_gt))
    assert np.allclose(got, want, rtol=0, atol=1e-15), (got, want)
    # a wider cut-off takes in the ranks past 3; one past every rank takes in all; negative entries never hit
    assert hits_from_ranks(ranks, 6).sum(1).tolist() == [3, 1, 1]
    assert hits_from_ranks(ranks, 1000).sum(1).tolist() == [5, 1, 2]
    assert tuple(hits_from_ranks(ranks, 1000).shape) == (3, 1000)
