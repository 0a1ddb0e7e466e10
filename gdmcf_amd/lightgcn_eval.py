"""Ranking metrics of the LightGCN script (reference lightGCN.py:67-127) from the final embeddings, on the device.

`get_metrics` ranks with the fused score product + top-k (evaluate_utils.score_topk) and reads the hits off the lists;
`get_metrics_at` ranks once with evaluate_utils.score_rank and reads every cut-off's hits off the exact ranks of the test items
(`hits_from_ranks`).  Both put their hit matrix through `ranking_terms`, the reference's arithmetic in float64.  `_history_rows`
cuts the rows of the asked users out of a history or target CSR; LightGCN.recommend / rank_targets use it too.
"""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib


def _history_rows(history, ids):
    """(indptr int64, indices int32) on ids' device: the rows `ids` of `history` (scipy CSR or DeviceCSR), or (None, None)."""
    if history is None:
        return None, None
    from .data_utils import DeviceCSR
    if isinstance(history, DeviceCSR):
        hp = history.indptr.to(ids.device)
        beg, end = hp[ids], hp[ids + 1]
        ln = end - beg
        ip = torch.zeros(ids.numel() + 1, dtype=torch.int64, device=ids.device)
        torch.cumsum(ln, 0, out=ip[1:])
        pos = torch.arange(int(ip[-1]), device=ids.device) - torch.repeat_interleave(ip[:-1] - beg, ln)
        return ip, history.indices.to(ids.device)[pos].to(torch.int32)
    sub = sp.csr_matrix(history)[ids.cpu().numpy()]
    return (torch.from_numpy(sub.indptr.astype(np.int64)).to(ids.device),
            torch.from_numpy(sub.indices.astype(np.int32)).to(ids.device))


def ranking_terms(hit, n_gt):
    """Per-user (recall, precision, ndcg, map) terms of the reference's get_metrics (lightGCN.py:98-125) from the hit matrix
    `hit` [U, K] (hit[u, j] = the j-th recommendation of u is a test item) and the users' test-set sizes `n_gt` [U] (> 0):
    float64 tensors on hit's device (any device: this is the arithmetic get_metrics runs on the GPU)."""
    hit = hit.to(torch.float64)
    n_gt = n_gt.to(torch.float64)
    K = hit.shape[1]
    j = torch.arange(K, device=hit.device, dtype=torch.float64)
    gain = 1.0 / torch.log(j + 2.0)
    recall = hit.sum(1) / n_gt
    precision = hit.sum(1) / K
    idcg = ((j[None, :] < torch.clamp(n_gt, max=K)[:, None]).to(torch.float64) * gain).sum(1)
    ndcg = (hit * gain).sum(1) / idcg
    ap = (hit * torch.cumsum(hit, 1) / (j + 1.0)).sum(1) / n_gt
    return recall, precision, ndcg, ap


def _ranked_users(what, user_emb, item_emb, n_users, n_items, train_csr, test_csr):
    """What get_metrics and get_metrics_at (`what`: the caller, for the error text) rank: (ids, ip, ix, gt, n_gt) -- the users
    with at least one test interaction (int64, on the embeddings' device), their rows of `train_csr` (_history_rows), their rows
    of the canonical test CSR (scipy: duplicates summed, indices sorted) and those rows' lengths (int64, on the device)."""
    _lib.require_gpu(user_emb, "user embeddings")
    _lib.require_gpu(item_emb, "item embeddings")
    dev = user_emb.device
    test = sp.csr_matrix(test_csr).astype(np.float32)
    test.sum_duplicates()
    test.sort_indices()
    assert test.shape == (n_users, n_items) and user_emb.shape[0] == n_users and item_emb.shape[0] == n_items
    users = np.nonzero(np.diff(test.indptr) > 0)[0].astype(np.int64)
    if len(users) == 0:
        raise ValueError(f"{what}: no user has a test interaction")
    ids = torch.from_numpy(users).to(dev)
    ip, ix = _history_rows(train_csr, ids)
    gt = test[users]
    n_gt = torch.from_numpy(np.diff(gt.indptr).astype(np.int64)).to(dev)
    return ids, ip, ix, gt, n_gt


def get_metrics(user_emb, item_emb, n_users, n_items, train_csr, test_csr, K):
    """(recall, precision, ndcg, map) @K of reference lightGCN.py:67-127 from the final embeddings: the users with at least
    one test interaction are ranked over all items but their training ones (`train_csr`, `test_csr`: scipy CSR [n_users,
    n_items]), each metric is the plain mean over those users.  Ranking by the fused gdmcf_score_topk_f32 (no score matrix, no
    dense mask); the hit matrix and the per-user terms are float64 on the device, the ranked lists never reach the host."""
    from .evaluate_utils import score_topk
    ids, ip, ix, gt, n_gt = _ranked_users("get_metrics", user_emb, item_emb, n_users, n_items, train_csr, test_csr)
    dev = ids.device
    top = score_topk(user_emb, item_emb, K, ip, ix, user_ids=ids, check_ids=False)  # [U_test, K]; ids: rows of test_csr
    # membership: (row, item) keys of the ground truth are sorted (CSR order), the recommendations are looked up in them
    rows = np.repeat(np.arange(ids.numel(), dtype=np.int64), np.diff(gt.indptr))
    gkeys = torch.from_numpy(rows * n_items + gt.indices.astype(np.int64)).to(dev)
    pkeys = torch.arange(ids.numel(), device=dev, dtype=torch.int64)[:, None] * n_items + top
    pos = torch.searchsorted(gkeys, pkeys.reshape(-1)).clamp_(max=gkeys.numel() - 1)
    hit = (gkeys[pos] == pkeys.reshape(-1)).reshape(pkeys.shape)
    return tuple(float(t.mean()) for t in ranking_terms(hit, n_gt))


def hits_from_ranks(ranks, K):
    """The hit matrix [U, K] (bool) get_metrics forms from its lists, from RANKS instead: `ranks` integer [U, G] (any device), the
    0-based catalogue rank of each test item of the user, negative = no item there; hit[u, r] = True for every rank r < K.  (The
    r-th recommendation is a test item exactly when some test item has rank r.)"""
    ok = (ranks >= 0) & (ranks < K)
    hit = torch.zeros(ranks.shape[0], int(K), dtype=torch.bool, device=ranks.device)
    rows = torch.arange(ranks.shape[0], device=ranks.device)[:, None].expand_as(ranks)
    hit[rows[ok], ranks[ok].to(torch.int64)] = True
    return hit


def _check_Ks(Ks):
    Ks = [int(K) for K in Ks]
    if not Ks or Ks != sorted(set(Ks)) or Ks[0] < 1:
        raise ValueError("get_metrics_at: Ks must be ascending, non-empty and >= 1")
    return Ks


def get_metrics_at(user_emb, item_emb, n_users, n_items, train_csr, test_csr, Ks):
    """get_metrics at every cut-off of `Ks` (ascending) from ONE ranking pass: {K: (recall, precision, ndcg, map)}.  The users
    with test interactions are ranked once by the fused gdmcf_score_rank_f32 (evaluate_utils.score_rank: the exact rank of every
    test item, no score matrix, no list), and each K's hit matrix is read off the ranks (hits_from_ranks) and goes through
    ranking_terms as get_metrics' does: for K <= 1024 each tuple equals get_metrics(..., K) exactly.  No list bounds K here: any
    K >= 1, also above 1024 and above n_items."""
    from .evaluate_utils import score_rank
    Ks = _check_Ks(Ks)
    ids, ip, ix, gt, n_gt = _ranked_users("get_metrics_at", user_emb, item_emb, n_users, n_items, train_csr, test_csr)
    tp = torch.from_numpy(gt.indptr.astype(np.int64)).to(ids.device)
    tx = torch.from_numpy(gt.indices.astype(np.int32)).to(ids.device)
    ranks = score_rank(user_emb, item_emb, tp, tx, ip, ix, user_ids=ids, G=int(np.diff(gt.indptr).max()), check_ids=False)  # [U_test, G]
    return {K: tuple(float(t.mean()) for t in ranking_terms(hits_from_ranks(ranks, K), n_gt)) for K in Ks}

