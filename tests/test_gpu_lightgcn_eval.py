"""GPU (-m gpu): LightGCN ranking -- gdmcf_score_topk_f32 (score product fused with the masked top-k) behind
evaluate_utils.score_topk, LightGCN.recommend and lightgcn.get_metrics.

1. exact lists: integer embeddings make every partial sum exact in float32, so indices AND values must equal
   masked_topk on the materialised matrix (tie rule and degenerate-row convention pinned to the existing kernel's);
2. real-valued embeddings at the Yelp item count against float64 scores, inside the derived dot-product error bound;
3. the workspace bound and one full-size call;
4. LightGCN.recommend and get_metrics against score_topk and the numpy restatement of the reference's get_metrics."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib
from gdmcf_amd.evaluate_utils import masked_topk, score_topk
from tests.test_host_lightgcn_eval import np_get_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
YELP_U, YELP_I = 54574, 34395


def random_mask(rng, n_rows, n_items, mean_len, full_rows=(), keep=0):
    """CSR mask (indptr int64, indices int32, sorted rows): ~mean_len random items per row; the rows in `full_rows` mask all
    but `keep` items."""
    ip, ix = [0], []
    for r in range(n_rows):
        if r in full_rows:
            cols = np.sort(rng.choice(n_items, n_items - keep, replace=False))
        else:
            cols = np.sort(rng.choice(n_items, min(n_items, int(rng.poisson(mean_len))), replace=False))
        ix.append(cols)
        ip.append(ip[-1] + len(cols))
    return np.asarray(ip, dtype=np.int64), np.concatenate(ix).astype(np.int32)


@pytest.mark.parametrize("k", [1, 20, 100])
@pytest.mark.parametrize("n_items", [1000, 4099])
@pytest.mark.parametrize("d", [8, 64, 100, 1000])
def test_exact_lists_equal_masked_topk_on_the_materialised_matrix(d, n_items, k):
    rng = np.random.default_rng(1000 * d + n_items + k)
    n_users = 150  # two tiles of 64 rows and a ragged one
    ue = rng.integers(-4, 5, (n_users, d)).astype(np.float32)
    ie = rng.integers(-4, 5, (n_items, d)).astype(np.float32)
    ue[[3, 64, 149]] = 0.0  # every score of these users ties
    assert 16 * d < 2 ** 24
    scores = (ue.astype(np.float64) @ ie.astype(np.float64).T).astype(np.float32)  # exact
    ue_d, ie_d, sc_d = (torch.from_numpy(a).to(DEV) for a in (ue, ie, scores))
    picked = np.sort(rng.choice(n_users, 77, replace=False))
    picked[:3] = [3, 64, 149]  # (ids need not be sorted or unique)
    for ids in (None, picked):
        rows = np.arange(n_users) if ids is None else ids
        n_rows = len(rows)
        # rows 1 and n_rows - 1 keep fewer than k items unmasked (k = 1: none at all); row 0 is an all-tie row with a mask
        ip, ix = random_mask(rng, n_rows, n_items, 30, full_rows=(1, n_rows - 1), keep=max(k - 3, 0))
        ip_d, ix_d = torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV)
        ids_d = None if ids is None else torch.from_numpy(ids.astype(np.int64)).to(DEV)
        want_v, want_i = masked_topk(sc_d[torch.from_numpy(rows).to(DEV)].contiguous(), k, ip_d, ix_d, return_values=True)
        got_v, got_i = score_topk(ue_d, ie_d, k, ip_d, ix_d, user_ids=ids_d, return_values=True)
        assert got_i.shape == (n_rows, k) and got_i.dtype == torch.int64 and got_v.dtype == torch.float32
        assert torch.equal(got_i, want_i), (d, n_items, k, ids is None)
        assert torch.equal(got_v, want_v)
        assert torch.equal(score_topk(ue_d, ie_d, k, ip_d, ix_d, user_ids=ids_d), want_i)  # indices-only convention
    # no mask at all
    want_i = masked_topk(sc_d, k)
    assert torch.equal(score_topk(ue_d, ie_d, k), want_i)


@pytest.mark.parametrize("d,k", [(8, 100), (8, 160), (8, 300), (8, 416), (8, 1000), (7, 100), (66, 20), (66, 1000), (1, 7)])
def test_exact_lists_with_rising_scores_every_tile_height_and_unaligned_d(d, k):
    """Rows whose scores rise with the item index pass the running bound at EVERY item, so their candidate lists fill as fast
    as they can: 64 appends per step, a compaction as soon as k + 64 more would not fit (k = 160, 416: at every step).  k picks
    the tile height (64 rows to k = 160, 32 to 416, 8 to 1024); d = 7, 66, 1 take the scalar loads (d % 4 != 0) and the padded
    k loop.  Integer embeddings again (|score| <= 4 * 4098 + 16 d < 2^24: exact), compared with masked_topk."""
    rng = np.random.default_rng(100 * d + k)
    n_users, n_items = 70, 4099
    ue = rng.integers(-4, 5, (n_users, d)).astype(np.float32)
    ie = rng.integers(-4, 5, (n_items, d)).astype(np.float32)
    ie[:, 0] = np.arange(n_items)                    # column 0: the item index
    ue[:, 0] = rng.integers(-1, 2, n_users)          # so most rows carry a ramp under the random part
    hot = np.zeros((6, d), np.float32)
    hot[:, 0] = [1, 4, -1, -4, 1, 1]                 # pure ramps: users 0, 5, 64, 69 strictly rising, 17 and 33 strictly falling
    ue[[0, 5, 17, 33, 64, 69]] = hot
    if d >= 7:
        ie[:, 1] = np.arange(n_items) % 64           # column 1: rising inside each 64-item step, equal from step to step
        ue[[2, 40, 66]] = 0.0
        ue[[2, 40, 66], 1] = [1, 3, 1]
        ue[66, 0] = 1                                # (row 66: ramp + sawtooth)
    assert 4 * (n_items - 1) + 16 * d < 2 ** 24
    scores = (ue.astype(np.float64) @ ie.astype(np.float64).T).astype(np.float32)  # exact
    ue_d, ie_d, sc_d = (torch.from_numpy(a).to(DEV) for a in (ue, ie, scores))
    want_v, want_i = masked_topk(sc_d, k, return_values=True)
    got_v, got_i = score_topk(ue_d, ie_d, k, return_values=True)
    bad = (got_i != want_i).any(1).nonzero().flatten().tolist()
    assert not bad, f"rows with a different list: {bad}"
    assert torch.equal(got_v, want_v)
    ip, ix = random_mask(rng, n_users, n_items, 300, full_rows=(1, 64), keep=max(k - 3, 0))
    ip_d, ix_d = torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV)
    want_v, want_i = masked_topk(sc_d, k, ip_d, ix_d, return_values=True)
    got_v, got_i = score_topk(ue_d, ie_d, k, ip_d, ix_d, return_values=True)
    assert torch.equal(got_i, want_i) and torch.equal(got_v, want_v)
    again_v, again_i = score_topk(ue_d, ie_d, k, ip_d, ix_d, return_values=True)
    assert torch.equal(got_i, again_i) and torch.equal(got_v.view(torch.int32), again_v.view(torch.int32))  # same bits


def test_exact_lists_from_item_slabs_at_the_middle_tile_height():
    """Few rows and many items: the items are cut into slabs and merged (workspace > 0), here with the 32-row tile (k = 300)."""
    rng = np.random.default_rng(300)
    n_users, n_items, d, k = 40, 30000, 8, 300
    assert _lib.load().gdmcf_score_topk_ws_bytes(n_users, n_items, d, k) > 0
    ue = rng.integers(-4, 5, (n_users, d)).astype(np.float32)
    ie = rng.integers(-4, 5, (n_items, d)).astype(np.float32)
    ie[:, 0] = np.arange(n_items)
    ue[:, 0] = rng.integers(-1, 2, n_users)
    ue[[0, 39]] = 0.0
    ue[[0, 39], 0] = 1  # strictly rising rows
    scores = (ue.astype(np.float64) @ ie.astype(np.float64).T).astype(np.float32)  # exact: < 2^24
    ue_d, ie_d, sc_d = (torch.from_numpy(a).to(DEV) for a in (ue, ie, scores))
    ip, ix = random_mask(rng, n_users, n_items, 300)
    ip_d, ix_d = torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV)
    want_v, want_i = masked_topk(sc_d, k, ip_d, ix_d, return_values=True)
    got_v, got_i = score_topk(ue_d, ie_d, k, ip_d, ix_d, return_values=True)
    assert torch.equal(got_i, want_i) and torch.equal(got_v, want_v)


def xavier(rng, n, d):
    b = np.sqrt(6.0 / (n + d))
    return rng.uniform(-b, b, (n, d)).astype(np.float32)


def test_real_valued_embeddings_within_the_dot_product_error_bound():
    rng = np.random.default_rng(7)
    d, k, n_rows = 64, 100, 1024
    ue, ie = xavier(rng, YELP_U, d), xavier(rng, YELP_I, d)
    ids = rng.choice(YELP_U, n_rows, replace=False).astype(np.int64)
    ip, ix = random_mask(rng, n_rows, YELP_I, 25.6)  # Yelp: 1.4 M training interactions over 54 574 users
    ue_d, ie_d = torch.from_numpy(ue).to(DEV), torch.from_numpy(ie).to(DEV)
    args = (ue_d, ie_d, k, torch.from_numpy(ip).to(DEV), torch.from_numpy(ix).to(DEV))
    val_d, idx_d = score_topk(*args, user_ids=torch.from_numpy(ids).to(DEV), return_values=True)
    val2_d, idx2_d = score_topk(*args, user_ids=torch.from_numpy(ids).to(DEV), return_values=True)
    assert torch.equal(idx_d, idx2_d) and torch.equal(val_d.view(torch.int32), val2_d.view(torch.int32))  # same bits
    val, idx = val_d.cpu().numpy().astype(np.float64), idx_d.cpu().numpy()
    u64 = ue[ids].astype(np.float64)
    v64 = ie.astype(np.float64)
    s = u64 @ v64.T
    eps = 2.0 * d * 2.0 ** -24 * (np.abs(u64) @ np.abs(v64).T)  # gamma_d doubled: derived, not measured
    masked = np.zeros((n_rows, YELP_I), dtype=bool)
    masked[np.repeat(np.arange(n_rows), np.diff(ip)), ix] = True
    rr = np.arange(n_rows)[:, None]
    worst_val = float(np.max(np.abs(val - s[rr, idx]) / eps[rr, idx]))
    print(f"max |value - s| / eps = {worst_val:.3f}")
    assert np.all(np.abs(val - s[rr, idx]) <= eps[rr, idx])
    assert not masked[rr, idx].any()
    assert all(len(set(row)) == k for row in idx.tolist())
    dv, di = np.diff(val, axis=1), np.diff(idx, axis=1)
    assert np.all(dv <= 0) and np.all(di[dv == 0] > 0)
    last = idx[:, -1]
    bound = s[np.arange(n_rows), last][:, None] + eps + eps[np.arange(n_rows), last][:, None]
    out = ~masked
    out[rr, idx] = False  # the unmasked items that were not returned
    worst_out = float(np.max(np.where(out, s - bound, -np.inf)))
    print(f"max over left-out items of s - bound = {worst_out:.3e}")
    assert np.all(s[out] <= bound[out])


def test_workspace_bound_and_one_full_size_call():
    lib = _lib.load()
    d, k = 64, 100
    assert lib.gdmcf_score_topk_ws_bytes(YELP_U, YELP_I, d, k) <= 0.05 * 4 * YELP_U * YELP_I
    rng = np.random.default_rng(11)
    ue_d = torch.from_numpy(xavier(rng, YELP_U, d)).to(DEV)
    ie_d = torch.from_numpy(xavier(rng, YELP_I, d)).to(DEV)
    ln = rng.poisson(25.6, YELP_U)
    ip = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    cols = rng.integers(0, YELP_I, int(ip[-1])).astype(np.int32)  # (unsorted, duplicates possible: both are allowed)
    ip_d, ix_d = torch.from_numpy(ip).to(DEV), torch.from_numpy(cols).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    val, idx = score_topk(ue_d, ie_d, k, ip_d, ix_d, return_values=True)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before <= 0.05 * 4 * YELP_U * YELP_I + 16 * YELP_U * k  # outputs + workspace only
    assert idx.shape == (YELP_U, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < YELP_I
    # no masked item: (row, item) keys of the mask, sorted, looked up for every returned item
    rows = torch.repeat_interleave(torch.arange(YELP_U, device=DEV), torch.from_numpy(ln).to(DEV))
    mkeys = torch.sort(rows * YELP_I + ix_d.to(torch.int64)).values
    pkeys = (torch.arange(YELP_U, device=DEV)[:, None] * YELP_I + idx).reshape(-1)
    pos = torch.searchsorted(mkeys, pkeys).clamp_(max=mkeys.numel() - 1)
    assert not bool((mkeys[pos] == pkeys).any())
    # no duplicate
    srt = torch.sort(idx, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())
    # non-increasing values, equal values in ascending index
    dv = val[:, 1:] - val[:, :-1]
    assert bool((dv <= 0).all())
    assert bool(((idx[:, 1:] > idx[:, :-1]) | (dv < 0)).all())


def small_split(rng, U, I, per_user, no_test_every):
    rows = np.repeat(np.arange(U), per_user)
    cols = rng.integers(0, I, U * per_user)
    held = rng.random(len(rows)) < 0.3
    held[rows % no_test_every == 0] = False  # these users have no test item: left out of the mean
    mk = lambda m: sp.csr_matrix((np.ones(int(m.sum()), np.float32), (rows[m], cols[m])), shape=(U, I))
    train, test = mk(~held), mk(held)
    for m in (train, test):
        m.sum_duplicates()
        m.data[:] = 1.0
    test = test - test.multiply(train)  # an interaction is in one split only
    test.eliminate_zeros()
    return train.tocsr(), test.tocsr()


def test_recommend_equals_score_topk_on_the_propagated_tables():
    from gdmcf_amd.data_utils import DeviceCSR
    rng = np.random.default_rng(3)
    U, I, d, k = 300, 211, 32, 10
    train, _ = small_split(rng, U, I, 12, 7)
    coo = train.tocoo()
    torch.manual_seed(0)
    lg = gdmcf_amd.LightGCN({"user_id_idx": coo.row, "item_id_idx": coo.col}, U, I, 2, d, device=DEV).to(DEV)
    users = rng.choice(U, 90, replace=False).astype(np.int64)
    with torch.no_grad():
        fu, fi, _, _ = lg.propagate_through_layers()
    sub = train[users]
    ip = torch.from_numpy(sub.indptr.astype(np.int64)).to(DEV)
    ix = torch.from_numpy(sub.indices.astype(np.int32)).to(DEV)
    want = score_topk(fu, fi, k, ip, ix, user_ids=torch.from_numpy(users).to(DEV))
    assert torch.equal(lg.recommend(users, k, history=train), want)
    assert torch.equal(lg.recommend(torch.from_numpy(users), k, history=DeviceCSR(train, DEV)), want)
    assert torch.equal(lg.recommend(users, k), score_topk(fu, fi, k, user_ids=torch.from_numpy(users).to(DEV)))
    assert E0_grad_untouched(lg)


def E0_grad_untouched(lg):
    return lg.E0.weight.grad is None and lg.E0.weight.requires_grad


@pytest.mark.parametrize("K", [5, 20])
def test_get_metrics_matches_the_numpy_restatement(K):
    from gdmcf_amd.lightgcn import get_metrics
    rng = np.random.default_rng(5 + K)
    U, I, d = 260, 180, 16
    train, test = small_split(rng, U, I, 10, 5)
    assert (np.diff(test.indptr) == 0).sum() >= U // 5  # users without test items
    # integer tables: the float32 scores are exact, so the device ranking is the float64 ranking (ties: lowest item first)
    ue = rng.integers(-3, 4, (U, d)).astype(np.float32)
    ie = rng.integers(-3, 4, (I, d)).astype(np.float32)
    want = np_get_metrics(ue, ie, train, test, K)
    got = get_metrics(torch.from_numpy(ue).to(DEV), torch.from_numpy(ie).to(DEV), U, I, train, test, K)
    print("get_metrics", got, "numpy", want)
    assert len(got) == 4
    assert np.all(np.abs(np.asarray(got) - np.asarray(want)) <= 1e-12), (got, want)
