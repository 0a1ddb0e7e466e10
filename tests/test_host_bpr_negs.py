"""CPU (-m "not gpu"): gdmcf_bpr_sample_pool_f32 refuses bad arguments before anything is launched, the host model of its
counter layout (tests/bpr_negs_ref.py) contains the one-negative draw as its (1, 1) case, the statistical conditions the GPU
test asserts hold for the model at the seeds it uses, and the new host API refuses CPU tensors."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib
from gdmcf_amd.lightgcn import BPRTrainer, sample_bpr_negatives
from tests import bpr_negs_ref as R
from tests import draws_ref as D


def test_sample_pool_entry_checks_its_arguments():
    """Every refused argument set returns before a launch (no GPU needed): the pointers are host addresses no kernel may see."""
    lib = _lib.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)

    def call(B=4, n_negs=1, pool=1, M=None, ldm=8, d=8, offset=0, ptrs=(p, p, p, p, p)):
        indptr, indices, users, pos, neg = ptrs
        return lib.gdmcf_bpr_sample_pool_f32(indptr, indices, users, B, n_negs, pool, 3, 5, M, ldm, d, 0, offset, pos, neg, None, None)

    for kw in (dict(B=0), dict(n_negs=0), dict(pool=0), dict(B=-1), dict(n_negs=1 << 10, pool=1 << 10), dict(n_negs=1 << 20),
               dict(pool=2, M=p, d=0), dict(pool=2, M=p, ldm=7, d=8), dict(M=p, d=0), dict(offset=1 << 56)):
        assert call(**kw) == _lib.E_SHAPE, kw
    for k in range(5):
        ptrs = tuple(None if i == k else p for i in range(5))
        assert call(ptrs=ptrs) == _lib.E_ARG, k
    assert call(pool=2, M=None) == _lib.E_ARG
    assert call(n_negs=3, pool=4, M=None, d=0) == _lib.E_ARG
    assert call(ptrs=(None,) * 5) == _lib.E_ARG  # the pattern of test_bpr_entry_points_check_their_arguments


@pytest.mark.parametrize("offset", [0, 9, (1 << 32) + 3])
def test_host_model_contains_the_one_negative_draw(offset):
    indptr, indices, U, It, users = R.edge_graph()
    pos0, neg0, flag0 = D.bpr_triples(indptr, indices, users, U, It, 13, offset)
    pos, neg, flag, cands = R.pool_triples(indptr, indices, users, U, It, 13, offset, 1, 1)
    assert np.array_equal(pos, pos0) and np.array_equal(neg[:, 0], neg0) and flag == flag0 == 1
    assert np.array_equal(cands[:, 0, 0], neg0)
    # more slots or a pool leave slot 0's first candidate, and the positive, where they were
    pos3, neg3, _, cands3 = R.pool_triples(indptr, indices, users, U, It, 13, offset, 3, 1)
    assert np.array_equal(pos3, pos0) and np.array_equal(neg3[:, 0], neg0)
    zeros = np.zeros((U + It, 4), np.float32)
    assert np.array_equal(R.pool_triples(indptr, indices, users, U, It, 13, offset, 1, 4, zeros)[3][:, 0, 0], neg0)
    assert [R.candidate_place(q) for q in (0, 2, 3, 6, 7, 14)] == [(0, 1), (0, 3), (1, 0), (1, 3), (2, 0), (3, 3)]


def test_edge_graph_is_what_the_gpu_test_needs():
    indptr, indices, U, It, users = R.edge_graph()
    deg = np.diff(indptr)
    assert (U, It) == (37, 53) and deg[3] == 52 and deg[5] == 1 and deg[7] == 0 and deg[11] == 53
    rest = np.delete(deg, [3, 5, 7, 11])
    assert rest.min() >= 1 and rest.max() <= 6
    assert users.shape == (33,) and len(np.unique(users)) < 33 and (users == U).any()
    _, neg, flag, _ = R.pool_triples(indptr, indices, users, U, It, 13, 0, 3, 1)
    assert flag == 1 and (neg[users == 3] == 17).all() and (neg[np.isin(users, [7, 11, U])] == -1).all()


def test_statistical_conditions_hold_for_the_host_model():
    """The GPU test asserts these on the kernel's output, which must equal the model's: same seeds, same offsets."""
    indptr, indices, U, It, users = R.property_graph()
    _, neg, flag, _ = R.pool_triples(indptr, indices, users, U, It, 3, 0, 3, 1)
    assert flag == 0 and neg.shape == (2000, 3)
    R.check_uniform_negatives(users, neg)
    M = R.increasing_score_table(U, It, 8)
    _, neg, flag, cands = R.pool_triples(indptr, indices, users, U, It, 3, 1, 3, 3, M)
    assert flag == 0
    R.check_best_of_three(users, neg, cands)


def test_ties_keep_the_earliest_drawn_and_nan_never_replaces():
    indptr, indices, U, It, users = R.edge_graph()
    M = np.zeros((U + It, 4), np.float32)  # every score equal
    _, neg, _, cands = R.pool_triples(indptr, indices, users, U, It, 13, 0, 2, 5, M)
    assert np.array_equal(neg, cands[:, :, 0])
    M[:] = np.nan
    assert np.array_equal(R.pool_triples(indptr, indices, users, U, It, 13, 0, 2, 5, M)[1], cands[:, :, 0])


def test_negatives_have_no_cpu_fallback():
    N, U, d = 10, 4, 8
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample_bpr_negatives(torch.zeros(U + 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), ids, N - U, 0, 0, n_negs=2,
                             pool=3, M=torch.zeros(N, d))
    uu, ii = np.array([0, 1, 2, 3]), np.array([0, 1, 2, 3])
    m = gdmcf_amd.LightGCN({"user_id_idx": uu, "item_id_idx": ii}, U, N - U, 1, d, device="cpu")
    Rm = sp.csr_matrix((np.ones(4, np.float32), (uu, ii)), shape=(U, N - U))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BPRTrainer(m, Rm, n_negs=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BPRTrainer(m, Rm, n_negs=0, neg_pool=0)  # (the GPU requirement is checked first)
