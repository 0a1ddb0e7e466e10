"""CPU (-m "not gpu"): the LightGCN ranking surface -- gdmcf_score_topk_f32 / gdmcf_score_topk_ws_bytes check their arguments
(their declaration, export and binding: tests/test_host_abi.py); the ranking metrics of the reference's get_metrics
(lightGCN.py:98-125), restated here in numpy from their definitions, and the package's own per-user terms reproduce a case
worked out by hand; the product path refuses CPU tensors."""
import math

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib


def np_metrics_from_lists(top, gt_lists):
    """(recall, precision, ndcg, map): `top` [U, K] ranked item ids, gt_lists[u] the (non-empty) test items of user u.
    hit_j = [top_j in GT]; recall = sum hit / |GT|; precision = sum hit / K; ndcg = sum_j hit_j / ln(j + 2) over
    sum_{j < min(|GT|, K)} 1 / ln(j + 2); map = sum_j hit_j cumsum(hit)_j / (j + 1) over |GT|; plain means over the users."""
    top = np.asarray(top)
    U, K = top.shape
    rec, pre, ndcg, ap = [], [], [], []
    for u in range(U):
        gt = set(int(x) for x in gt_lists[u])
        hit = np.array([1.0 if int(x) in gt else 0.0 for x in top[u]], dtype=np.float64)
        rec.append(hit.sum() / len(gt))
        pre.append(hit.sum() / K)
        dcg = sum(hit[j] / math.log(j + 2) for j in range(K))
        idcg = sum(1.0 / math.log(j + 2) for j in range(min(len(gt), K)))
        ndcg.append(dcg / idcg)
        cs = np.cumsum(hit)
        ap.append(sum(hit[j] * cs[j] / (j + 1) for j in range(K)) / len(gt))
    return float(np.mean(rec)), float(np.mean(pre)), float(np.mean(ndcg)), float(np.mean(ap))


def np_get_metrics(user_emb, item_emb, train_csr, test_csr, K):
    """The reference's get_metrics restated: float64 scores, -inf on the training interactions, the K best per user (equal
    scores: lowest item first), over the users with at least one test interaction."""
    s = np.asarray(user_emb, dtype=np.float64) @ np.asarray(item_emb, dtype=np.float64).T
    tr = train_csr.tocsr()
    te = test_csr.tocsr()
    users = np.nonzero(np.diff(te.indptr) > 0)[0]
    top, gts = [], []
    for u in users:
        row = s[u].copy()
        row[tr.indices[tr.indptr[u]:tr.indptr[u + 1]]] = -np.inf
        top.append(np.argsort(-row, kind="stable")[:K])
        gts.append(te.indices[te.indptr[u]:te.indptr[u + 1]])
    return np_metrics_from_lists(np.stack(top), gts)


def test_score_topk_rejects_bad_arguments_without_a_gpu():
    """Argument checks run before any launch, with the codes of gdmcf_topk_masked_f32: shape -> E_SHAPE, k > 1024 -> E_ARG."""
    f = _lib.load().gdmcf_score_topk_f32
    assert f(None, 64, None, 0, None, 64, 100, 64, None, None, 5, None, None, None, 0, None) == _lib.E_SHAPE  # no rows
    assert f(None, 64, None, 8, None, 64, 100, 64, None, None, 101, None, None, None, 0, None) == _lib.E_SHAPE  # k > n_items
    assert f(None, 64, None, 8, None, 64, 100, 64, None, None, 0, None, None, None, 0, None) == _lib.E_SHAPE  # k < 1
    assert f(None, 64, None, 8, None, 64, 5000, 64, None, None, 1025, None, None, None, 0, None) == _lib.E_ARG  # k > 1024
    assert f(None, 8192, None, 8, None, 8192, 5000, 4097, None, None, 5, None, None, None, 0, None) == _lib.E_ARG  # d > 4096


def test_score_topk_workspace_is_a_sliver_of_the_score_matrix():
    """Yelp shape, k = 100: at most 5 % of the 4 U I bytes the score matrix would take; few rows: still at most 5 %."""
    ws = _lib.load().gdmcf_score_topk_ws_bytes
    assert ws(54574, 34395, 64, 100) <= 0.05 * 4 * 54574 * 34395
    assert ws(1024, 34395, 64, 100) <= 0.05 * 4 * 1024 * 34395
    assert ws(400, 94949, 64, 100) <= 0.05 * 4 * 400 * 94949


def _hand_case():
    # K = 3.  user 0: |GT| = 5 > K, hits at ranks 0 and 2; user 1: one test item, hit at rank 1; user 2: no hit
    top = np.array([[1, 9, 2], [0, 7, 3], [1, 2, 3]])
    gts = [[1, 2, 3, 4, 5], [7], [4, 6]]
    l2, l3, l4 = math.log(2), math.log(3), math.log(4)
    recall = (2 / 5 + 1 + 0) / 3
    precision = (2 / 3 + 1 / 3 + 0) / 3
    ndcg = ((1 / l2 + 1 / l4) / (1 / l2 + 1 / l3 + 1 / l4) + (1 / l3) / (1 / l2) + 0) / 3
    ap = ((1 * 1 / 1 + 2 * 1 / 3) / 5 + (1 * 1 / 2) / 1 + 0) / 3
    return top, gts, (recall, precision, ndcg, ap)


def test_numpy_restatement_reproduces_the_hand_worked_case():
    top, gts, want = _hand_case()
    got = np_metrics_from_lists(top, gts)
    assert np.allclose(got, want, rtol=0, atol=1e-15), (got, want)


def test_ranking_terms_reproduce_the_hand_worked_case():
    """gdmcf_amd.lightgcn.ranking_terms is the arithmetic get_metrics applies to the device's hit matrix."""
    from gdmcf_amd.lightgcn import ranking_terms
    top, gts, want = _hand_case()
    hit = torch.tensor([[int(x) in set(g) for x in row] for row, g in zip(top, gts)])
    n_gt = torch.tensor([len(g) for g in gts])
    terms = ranking_terms(hit, n_gt)
    assert all(t.dtype == torch.float64 for t in terms)
    got = tuple(float(t.mean()) for t in terms)
    assert np.allclose(got, want, rtol=0, atol=1e-15), (got, want)
    assert float(terms[0][2]) == 0.0 and float(terms[2][2]) == 0.0  # the user without a hit


def test_score_topk_refuses_cpu_tensors():
    import gdmcf_amd
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        gdmcf_amd.score_topk(torch.zeros(4, 8), torch.zeros(9, 8), 2)
    from gdmcf_amd.lightgcn import get_metrics
    import scipy.sparse as sp
    with pytest.raises(RuntimeError, match="must live on the MI355X"):
        get_metrics(torch.zeros(4, 8), torch.zeros(9, 8), 4, 9, sp.csr_matrix((4, 9)), sp.csr_matrix((4, 9)), 2)
