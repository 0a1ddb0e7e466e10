"""CPU (-m "not gpu"): the fused BPR step's C entry points check their arguments (their declaration, export and binding:
tests/test_host_abi.py), its host API refuses CPU tensors, and the sampler's "r-th item missing from a sorted row" search
(csrc/bpr.hip: bpr_sample_kernel) is right on paper."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib
from gdmcf_amd.lightgcn import BPRTrainer, bpr_loss_grad, bpr_reg_grad_, sample_bpr_items


def test_bpr_entry_points_check_their_arguments():
    """Argument errors are reported before anything is launched (no GPU needed)."""
    lib = _lib.load()
    assert lib.gdmcf_bpr_sample_f32(None, None, None, 4, 3, 5, 0, 0, None, None, None, None) == _lib.E_ARG
    assert lib.gdmcf_bpr_loss_f32(None, 8, None, 8, 8, None, None, None, 0, 3, 5, None, None, None, None, None, None) == _lib.E_SHAPE
    assert lib.gdmcf_bpr_grad_f32(2, None, None, None, None, 4, 3, 5, None, None, 8, 8, None, 8, 0.0, None, 0, None) == _lib.E_ARG


def test_bpr_has_no_cpu_fallback():
    N, U, d = 10, 4, 8
    M, E0 = torch.zeros(N, d), torch.zeros(N, d)
    ids = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bpr_loss_grad(M, E0, ids, ids, ids, U, 1e-4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bpr_reg_grad_(M, E0, ids, ids, ids, U, 1e-4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sample_bpr_items(torch.zeros(U + 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), ids, N - U, 0, 0)
    uu, ii = np.array([0, 1, 2, 3]), np.array([0, 1, 2, 3])
    m = gdmcf_amd.LightGCN({"user_id_idx": uu, "item_id_idx": ii}, U, N - U, 1, d, device="cpu")
    R = sp.csr_matrix((np.ones(4, np.float32), (uu, ii)), shape=(U, N - U))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BPRTrainer(m, R)


def nth_missing(row, r):
    """The kernel's search, restated: row sorted and distinct; the r-th (from 0) item that is not in it."""
    lo, hi = 0, len(row)
    while lo < hi:
        mid = (lo + hi) >> 1
        if row[mid] - mid > r:
            hi = mid
        else:
            lo = mid + 1
    return r + lo


def test_nth_missing_item_search_matches_brute_force():
    rng = np.random.default_rng(0)
    cases = [(12, [0]), (12, [11]), (12, [0, 1, 2]), (12, [9, 10, 11]), (12, list(range(11))), (12, list(range(1, 12))),
             (12, [0, 11]), (2, [0]), (2, [1]), (7, [0, 2, 4, 6]), (7, [1, 3, 5])]
    for _ in range(200):
        n = int(rng.integers(2, 60))
        deg = int(rng.integers(1, n))
        cases.append((n, sorted(rng.choice(n, size=deg, replace=False).tolist())))
    for n, row in cases:
        missing = [i for i in range(n) if i not in row]
        assert len(missing) == n - len(row) > 0
        # every r, so r = 0 and r = n - deg - 1 in particular
        assert [nth_missing(row, r) for r in range(len(missing))] == missing, (n, row)
