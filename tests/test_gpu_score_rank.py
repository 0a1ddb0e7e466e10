"""GPU (-m gpu): gdmcf_score_rank_f32 -- the exact ranks of named items from the fused score product -- behind
evaluate_utils.score_rank, LightGCN.rank_targets and lightgcn.get_metrics_at.

1. exact ranks: integer embeddings make every partial sum exact in float32, so ranks and n_live must equal gdmcf_rank_targets_f32
   on the materialised matrix, the -1 conventions included, at every product variant;
2. every tile height, passes, slabs, unaligned d and the loaded atomic path (ramps: nearly every score between a row's targets);
3. real-valued tables: the rank of an item is its place in score_topk's full list (a target scored in another summation order
   would count itself);
4. the Yelp item count against float64 scores inside the derived dot-product error bound;
5. LightGCN.rank_targets, get_metrics_at, rank_metrics_device on the ranks;
6. the error codes."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib, evaluate_utils
from gdmcf_amd.evaluate_utils import score_rank, score_topk
from tests.test_host_lightgcn_eval import np_get_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
YELP_U, YELP_I = 54574, 34395
FILL = -9  # what the output buffers hold before a launch


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def _csr_of(rows):
    """(indptr, indices) of hand-built rows: nothing is sorted, merged or range-checked."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(1, np.int32)])  # (never empty)


def random_mask_rows(rng, n_rows, n_items, mean_len, full_rows=(), keep=0):
    """Mask rows: ~mean_len random items each, unsorted, with a repeat and the out-of-range entries -1 and n_items in some; the
    rows in `full_rows` mask all but `keep` items."""
    rows = []
    for r in range(n_rows):
        if r in full_rows:
            cols = rng.permutation(n_items)[:n_items - keep]
        else:
            cols = rng.choice(n_items, min(n_items, int(rng.poisson(mean_len))), replace=False)
            if r % 5 == 2 and len(cols):
                cols = np.concatenate([cols, cols[:1], [-1, n_items]])
        rows.append(cols.astype(np.int64))
    return rows


def target_rows(rng, n_rows, n_items, G, mask_rows=None, spread=False):
    """Target rows of length 0 .. G (spread: mostly G, drawn without repeats across the catalogue); row 0 empty, row 1 one item,
    row 2 exactly G with a repeat, row 3 with -1, n_items and n_items + 7 inside, row 4 its own masked items first, row 5 longer
    than G."""
    rows = []
    for r in range(n_rows):
        n = G if (spread and r % 3) else int(rng.integers(0, G + 1))
        rows.append(rng.choice(n_items, n, replace=False) if n <= n_items else rng.integers(0, n_items, n))
    rows[0] = np.zeros(0, dtype=np.int64)
    rows[1] = rng.integers(0, n_items, 1)
    two = rng.integers(0, n_items, G)
    two[-1] = two[0]
    rows[2] = two
    rows[3] = np.concatenate([[-1], rng.integers(0, n_items, 2), [n_items], rng.integers(0, n_items, 1), [n_items + 7]])[:max(G, 1)]
    if mask_rows is not None:
        own = np.asarray([c for c in mask_rows[4] if 0 <= c < n_items][:3], dtype=np.int64)
        rows[4] = np.concatenate([own, rng.integers(0, n_items, 2)])[:max(G, 1)]
        last = n_rows - 1  # (a row that masks nearly everything: masked and unmasked targets)
        rows[last] = rng.integers(0, n_items, min(G, 6))
    rows[5] = rng.integers(0, n_items, G + 5)
    return [np.asarray(r, dtype=np.int64) for r in rows]


def fused(ue_d, ie_d, ids, mask, tgt, G, pad=2, live=True):
    """gdmcf_score_rank_f32 through its C entry: (ranks [n_rows, G + pad] pre-filled with FILL, n_live [n_rows]) on the host"""
    lib = _lib.load()
    n_rows = len(ids) if ids is not None else ue_d.shape[0]
    I, d = ie_d.shape
    out = torch.full((n_rows, G + pad), FILL, dtype=torch.int32, device=DEV)
    n_live = torch.full((n_rows,), FILL, dtype=torch.int32, device=DEV) if live else None
    ids_d = _t(ids, torch.int64)
    ip, ix = (_t(mask[0], torch.int64), _t(mask[1], torch.int32)) if mask is not None else (None, None)
    tp, tx = _t(tgt[0], torch.int64), _t(tgt[1], torch.int32)
    nbytes = int(lib.gdmcf_score_rank_ws_bytes(n_rows, I, d, G))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gdmcf_score_rank_f32(ue_d.data_ptr(), ue_d.stride(0), _lib.ptr(ids_d), n_rows, ie_d.data_ptr(), ie_d.stride(0), I, d,
                                        _lib.ptr(ip), _lib.ptr(ix), tp.data_ptr(), tx.data_ptr(), G, out.data_ptr(), out.stride(0),
                                        _lib.ptr(n_live), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), (n_live.cpu().numpy() if live else None)


def on_matrix(sc_d, mask, tgt, G):
    """gdmcf_rank_targets_f32 on stored rows with the same CSRs and rows = NULL: (ranks [B, G], n_live [B]) on the host"""
    B, I = sc_d.shape
    out = torch.full((B, G), FILL, dtype=torch.int32, device=DEV)
    n_live = torch.full((B,), FILL, dtype=torch.int32, device=DEV)
    ip, ix = (_t(mask[0], torch.int64), _t(mask[1], torch.int32)) if mask is not None else (None, None)
    tp, tx = _t(tgt[0], torch.int64), _t(tgt[1], torch.int32)
    _lib.check(_lib.load().gdmcf_rank_targets_f32(sc_d.data_ptr(), sc_d.stride(0), B, I, _lib.ptr(ip), _lib.ptr(ix), None, None,
                                                  tp.data_ptr(), tx.data_ptr(), None, G, out.data_ptr(), out.stride(0),
                                                  n_live.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), n_live.cpu().numpy()


def exact_scores(ue, ie):
    """The materialised matrix of integer tables: float64 product, cast (exact), and + 0.0 so that a -0 becomes the +0 the MFMA
    accumulator yields."""
    return (ue.astype(np.float64) @ ie.astype(np.float64).T).astype(np.float32) + np.float32(0.0)


def plan(n_rows, n_items, G):
    """(rows of a tile, targets of a pass, passes, item slabs) of gdmcf_debug_score_rank_plan"""
    v = [ctypes.c_int() for _ in range(4)]
    assert _lib.load().gdmcf_debug_score_rank_plan(n_rows, n_items, G, *[ctypes.byref(x) for x in v]) == 1
    return tuple(x.value for x in v)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact ranks at every product variant
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", [1000, 4099])
@pytest.mark.parametrize("d", [8, 64, 100, 1000])
def test_exact_ranks_equal_rank_targets_on_the_materialised_matrix(d, n_items):
    rng = np.random.default_rng(1000 * d + n_items)
    n_users, G = 150, 12  # two tiles of 64 rows and a ragged one
    ue = rng.integers(-4, 5, (n_users, d)).astype(np.float32)
    ie = rng.integers(-4, 5, (n_items, d)).astype(np.float32)
    ue[[3, 64, 149]] = 0.0  # every score of these users ties
    assert 16 * d < 2 ** 24
    scores = exact_scores(ue, ie)
    ue_d, ie_d, sc_d = (torch.from_numpy(a).to(DEV) for a in (ue, ie, scores))
    picked = np.sort(rng.choice(n_users, 77, replace=False))
    picked[:3] = [3, 64, 149]  # (ids need not be sorted or unique)
    for ids in (None, picked):
        rows = np.arange(n_users) if ids is None else ids
        n_rows = len(rows)
        mrows = random_mask_rows(rng, n_rows, n_items, 30, full_rows=(n_rows - 1,), keep=4)  # row 0: an all-tie row with a mask
        trows = target_rows(rng, n_rows, n_items, G, mrows)
        assert max(len(t) for t in trows) > G and min(len(t) for t in trows) == 0
        mask, tgt = _csr_of(mrows), _csr_of(trows)
        sub = sc_d[torch.from_numpy(rows).to(DEV)].contiguous()
        want, want_live = on_matrix(sub, mask, tgt, G)
        got, live = fused(ue_d, ie_d, ids, mask, tgt, G)
        assert np.array_equal(got[:, :G], want), (d, n_items, ids is None, np.argwhere(got[:, :G] != want)[:5])
        assert (got[:, G:] == FILL).all()  # the columns from G up to ldr are not written
        assert np.array_equal(live, want_live)
        assert (want[0] == -1).all() and (want[3][[0, 3, 5]] == -1).all() and (want >= 0).any()
        # the Python surface: the same tensor
        ids_d = None if ids is None else _t(ids, torch.int64)
        r2, l2 = score_rank(ue_d, ie_d, _t(tgt[0], torch.int64), _t(tgt[1], torch.int32), _t(mask[0], torch.int64),
                            _t(mask[1], torch.int32), user_ids=ids_d, G=G, return_live=True)
        assert r2.dtype == torch.int32 and r2.is_cuda and tuple(r2.shape) == (n_rows, G)
        assert np.array_equal(r2.cpu().numpy(), want) and np.array_equal(l2.cpu().numpy(), want_live)
    # no mask at all; G taken from the longest row
    trows = target_rows(rng, n_users, n_items, G)
    tgt = _csr_of(trows)
    want, want_live = on_matrix(sc_d, None, tgt, G + 5)
    got, live = fused(ue_d, ie_d, None, None, tgt, G + 5)
    assert np.array_equal(got[:, :G + 5], want) and (live == n_items).all() and np.array_equal(live, want_live)
    r3 = score_rank(ue_d, ie_d, _t(tgt[0], torch.int64), _t(tgt[1][:tgt[0][-1]], torch.int32))
    assert tuple(r3.shape) == (n_users, G + 5) and np.array_equal(r3.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. every tile height, passes, slabs, unaligned d, the loaded atomic path
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_boundaries(n_rows, n_items):
    """The last G of every class of the plan: where the tile height changes, and where a second pass begins."""
    out = []
    for G in range(1, 1100):
        a, b = plan(n_rows, n_items, G), plan(n_rows, n_items, G + 1)
        if a[0] != b[0] or (a[2] == 1 and b[2] == 2):
            out.append(G)
    return out


def ramp_tables(rng, n_users, n_items, d):
    """test_exact_lists_with_rising_scores...'s tables: column 0 of the items is the item index, so rows rise or fall with it."""
    ue = rng.integers(-4, 5, (n_users, d)).astype(np.float32)
    ie = rng.integers(-4, 5, (n_items, d)).astype(np.float32)
    ie[:, 0] = np.arange(n_items)
    ue[:, 0] = rng.integers(-1, 2, n_users)
    pure = [r for r in (0, 5, 17, 33, 64, 69) if r < n_users]
    ue[pure] = 0.0
    ue[pure, 0] = [1, 4, -1, -4, 1, 1][:len(pure)]  # pure ramps: strictly rising or falling
    if d >= 7:
        ie[:, 1] = np.arange(n_items) % 64
        saw = [r for r in (2, 40, 66) if r < n_users]
        ue[saw] = 0.0
        ue[saw, 1] = [1, 3, 1][:len(saw)]
    assert 4 * (n_items - 1) + 64 * 4 + 16 * d < 2 ** 24
    return ue, ie


def check_twice(ue, ie, mrows, trows, G):
    ue_d, ie_d, sc_d = (torch.from_numpy(a).to(DEV) for a in (ue, ie, exact_scores(ue, ie)))
    tgt = _csr_of(trows)
    for mask in (None, _csr_of(mrows)):
        want, want_live = on_matrix(sc_d, mask, tgt, G)
        got, live = fused(ue_d, ie_d, None, mask, tgt, G, pad=3)
        bad = (got[:, :G] != want).any(1).nonzero()[0].tolist()
        assert not bad, f"rows with different ranks: {bad[:10]}"
        assert (got[:, G:] == FILL).all() and np.array_equal(live, want_live)
        again, live2 = fused(ue_d, ie_d, None, mask, tgt, G, pad=3)
        assert np.array_equal(got, again) and np.array_equal(live, live2)  # run to run
    return want


CASES = [(8, "b0-1"), (8, "b0"), (8, "b0+1"), (8, "b1-1"), (8, "b1"), (8, "b1+1"), (8, "b2-1"), (8, "b2"), (8, "b2+1"),
         (7, "b0"), (66, "b1+1"), (66, "b2+1"), (1, "b0+1"), (66, "7"), (1, "7")]


@pytest.mark.parametrize("d,where", CASES)
def test_exact_ranks_with_ramps_every_tile_height_passes_and_unaligned_d(d, where):
    """G at and on both sides of every boundary of the plan (tile heights 64 / 32 / 16, the second pass), taken from the plan
    function itself; d = 7, 66, 1 take the scalar loads and the padded k loop.  Rising and falling rows with targets spread across
    the catalogue put nearly every score between two targets: every element is searched for and bumps a counter."""
    n_users, n_items = 70, 4099
    bs = plan_boundaries(n_users, n_items)
    assert len(bs) == 3, bs  # two changes of the tile height, then the second pass
    if where[0] == "b":
        G = bs[int(where[1])] + (int(where[2:]) if len(where) > 2 else 0)
    else:
        G = int(where)
    R, GP, npass, _ = plan(n_users, n_items, G)
    print(f"d={d} G={G}: tile of {R} rows, {GP} targets a pass, {npass} pass(es)")
    if where in ("b0", "b1", "b2"):
        nxt = plan(n_users, n_items, G + 1)
        assert nxt[0] != R or nxt[2] != npass
    rng = np.random.default_rng(100 * d + G)
    ue, ie = ramp_tables(rng, n_users, n_items, d)
    mrows = random_mask_rows(rng, n_users, n_items, 300, full_rows=(1, 64), keep=5)
    trows = target_rows(rng, n_users, n_items, G, mrows, spread=True)
    for r in (17, 33, 64):
        trows[r] = rng.choice(n_items, G, replace=False)  # (pure ramps with G targets spread over the catalogue)
    want = check_twice(ue, ie, mrows, trows, G)
    assert len(set(want[17].tolist())) == G  # a falling ramp: G distinct ranks


def test_exact_ranks_from_item_slabs():
    """Few rows and many items: the items are cut into slabs whose gap counts are added up by the finish launch."""
    n_users, n_items, d, G = 40, 30000, 8, 10
    lib = _lib.load()
    R, GP, npass, nslab = plan(n_users, n_items, G)
    assert nslab > 1 and npass == 1
    Gpad = -(-G // 16) * 16
    assert lib.gdmcf_score_rank_ws_bytes(n_users, n_items, d, G) == n_users * (8 * Gpad + 4 * nslab * (GP + 1) + 4 * nslab)
    rng = np.random.default_rng(300)
    ue, ie = ramp_tables(rng, n_users, n_items, d)
    mrows = random_mask_rows(rng, n_users, n_items, 300, full_rows=(7,), keep=3)
    trows = target_rows(rng, n_users, n_items, G, mrows, spread=True)
    check_twice(ue, ie, mrows, trows, G)
    # two passes from slabs, at the 16-row tile
    G2 = plan_boundaries(n_users, n_items)[2] + 1
    R2, _, npass2, nslab2 = plan(n_users, n_items, G2)
    assert (R2, npass2) == (16, 2) and nslab2 > 1
    check_twice(ue, ie, mrows, target_rows(rng, n_users, n_items, G2, mrows, spread=True), G2)


# ---------------------------------------------------------------------------------------------------------------------
# 3. real-valued tables agree with the top-k
# ---------------------------------------------------------------------------------------------------------------------
def xavier(rng, n, d):
    b = np.sqrt(6.0 / (n + d))
    return rng.uniform(-b, b, (n, d)).astype(np.float32)


@pytest.mark.parametrize("d", [64, 100])
def test_real_valued_ranks_are_the_positions_in_score_topks_list(d):
    """The materialised matrix cannot pin this (its rounding differs); score_topk's list is formed from the stream's own bits.  A
    target scored in another summation order would differ from its streamed self in the last bits, count itself or a neighbour,
    and be off by one."""
    rng = np.random.default_rng(d)
    n_users, n_items = 100, 1000
    ue, ie = xavier(rng, n_users, d), xavier(rng, n_items, d)
    ue_d, ie_d = torch.from_numpy(ue).to(DEV), torch.from_numpy(ie).to(DEV)
    mrows = random_mask_rows(rng, n_users, n_items, 30)
    trows = [rng.integers(0, n_items, 5) for _ in range(n_users)]
    for r in (0, 37, 99):
        trows[r] = rng.permutation(n_items)  # every item of these rows
    mask, tgt = _csr_of(mrows), _csr_of(trows)
    G = n_items
    ip, ix = _t(mask[0], torch.int64), _t(mask[1], torch.int32)
    idx = score_topk(ue_d, ie_d, n_items, ip, ix).cpu().numpy()
    assert (np.sort(idx, axis=1) == np.arange(n_items)).all()
    pos = np.argsort(idx, axis=1)  # pos[r, item] = place of the item in the full list
    got = score_rank(ue_d, ie_d, _t(tgt[0], torch.int64), _t(tgt[1], torch.int32), ip, ix, G=G).cpu().numpy()
    for r in range(n_users):
        t = trows[r]
        assert np.array_equal(got[r, :len(t)], pos[r, t]), (r, np.argwhere(got[r, :len(t)] != pos[r, t])[:5].tolist())
        assert (got[r, len(t):] == -1).all()
    assert sorted(got[37].tolist()) == list(range(n_items))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the Yelp item count against float64
# ---------------------------------------------------------------------------------------------------------------------
def test_yelp_item_count_within_the_dot_product_error_bound():
    """eps = 2 d 2^-24 |u|.|v| (gamma_d doubled: derived, not measured), as
    test_real_valued_embeddings_within_the_dot_product_error_bound: every rank lies between the number of unmasked items surely
    above the target and the number possibly at or above it."""
    rng = np.random.default_rng(7)
    d, n_rows, G = 64, 1024, 8
    ue, ie = xavier(rng, YELP_U, d), xavier(rng, YELP_I, d)
    ids = rng.choice(YELP_U, n_rows, replace=False).astype(np.int64)
    ln = np.minimum(rng.poisson(25.6, n_rows), YELP_I)
    mrows = [np.sort(rng.choice(YELP_I, int(n), replace=False)) for n in ln]  # Yelp: 1.4 M training interactions over 54 574 users
    tg = rng.integers(0, YELP_I, (n_rows, G))
    mask, tgt = _csr_of(mrows), _csr_of(list(tg))
    ue_d, ie_d = torch.from_numpy(ue).to(DEV), torch.from_numpy(ie).to(DEV)
    args = (ue_d, ie_d, _t(tgt[0], torch.int64), _t(tgt[1], torch.int32), _t(mask[0], torch.int64), _t(mask[1], torch.int32))
    r1, l1 = score_rank(*args, user_ids=_t(ids, torch.int64), G=G, return_live=True)
    r2, l2 = score_rank(*args, user_ids=_t(ids, torch.int64), G=G, return_live=True)
    assert torch.equal(r1, r2) and torch.equal(l1, l2)  # same bits
    ranks, live = r1.cpu().numpy().astype(np.int64), l1.cpu().numpy()
    assert np.array_equal(live, YELP_I - ln)
    u64 = ue[ids].astype(np.float64)
    v64 = ie.astype(np.float64)
    s = u64 @ v64.T
    eps = 2.0 * d * 2.0 ** -24 * (np.abs(u64) @ np.abs(v64).T)
    masked = np.zeros((n_rows, YELP_I), dtype=bool)
    masked[np.repeat(np.arange(n_rows), ln), mask[1][:mask[0][-1]]] = True
    rr = np.arange(n_rows)
    lo_side, hi_side = s - eps, s + eps
    lo_side[masked] = -np.inf  # a masked item is above no unmasked target
    hi_side[masked] = -np.inf
    n_masked_targets, worst = 0, 0
    for j in range(G):
        t = tg[:, j]
        st, et = s[rr, t], eps[rr, t]
        surely_above = (lo_side > (st + et)[:, None]).sum(1)
        maybe_above = (hi_side >= (st - et)[:, None]).sum(1)
        tm = masked[rr, t]
        # a masked target sits in the -inf tail by its index: exactly
        tail = live + np.array([np.searchsorted(mrows[r], t[r]) for r in range(n_rows)])
        n_masked_targets += int(tm.sum())
        assert np.array_equal(ranks[tm, j], tail[tm])
        ok = ~tm
        worst = max(worst, int((maybe_above - surely_above)[ok].max()))
        assert np.all(surely_above[ok] <= ranks[ok, j]) and np.all(ranks[ok, j] <= maybe_above[ok])
    print(f"widest bracket: {worst} places; masked targets: {n_masked_targets}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. model level
# ---------------------------------------------------------------------------------------------------------------------
def small_split(rng, U, I, per_user, no_test_every):
    rows = np.repeat(np.arange(U), per_user)
    cols = rng.integers(0, I, U * per_user)
    held = rng.random(len(rows)) < 0.3
    held[rows % no_test_every == 0] = False  # these users have no test item
    mk = lambda m: sp.csr_matrix((np.ones(int(m.sum()), np.float32), (rows[m], cols[m])), shape=(U, I))
    train, test = mk(~held), mk(held)
    for m in (train, test):
        m.sum_duplicates()
        m.data[:] = 1.0
    test = test - test.multiply(train)  # an interaction is in one split only
    test.eliminate_zeros()
    train, test = train.tocsr(), test.tocsr()
    train.sort_indices()
    test.sort_indices()
    return train, test


def test_lightgcn_rank_targets_equals_the_positions_in_recommends_full_list():
    from gdmcf_amd.data_utils import DeviceCSR
    rng = np.random.default_rng(3)
    U, I, d = 300, 211, 32
    train, test = small_split(rng, U, I, 12, 7)
    coo = train.tocoo()
    torch.manual_seed(0)
    lg = gdmcf_amd.LightGCN({"user_id_idx": coo.row, "item_id_idx": coo.col}, U, I, 2, d, device=DEV).to(DEV)
    users = rng.choice(U, 90, replace=False).astype(np.int64)
    users[:2] = [7, 7]  # (a repeat; user 7 has no test item)
    full = lg.recommend(users, I, history=train).cpu().numpy()
    pos = np.argsort(full, axis=1)
    G = int(np.diff(test[users].indptr).max())
    want = np.full((len(users), G), -1, dtype=np.int64)
    for b, u in enumerate(users):
        t = test.indices[test.indptr[u]:test.indptr[u + 1]]
        want[b, :len(t)] = pos[b, t]
    got, live = lg.rank_targets(users, test, history=train, return_live=True)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(users), G)
    assert np.array_equal(got.cpu().numpy(), want) and (want[0] == -1).all() and (want >= 0).any()
    assert np.array_equal(live.cpu().numpy(), I - np.diff(train[users].indptr))
    again = lg.rank_targets(torch.from_numpy(users), DeviceCSR(test, DEV), history=DeviceCSR(train, DEV))
    assert torch.equal(again, got)
    # no history: the training items are ranked too
    pos0 = np.argsort(lg.recommend(users, I).cpu().numpy(), axis=1)
    got0 = lg.rank_targets(users, test).cpu().numpy()
    for b, u in enumerate(users):
        t = test.indices[test.indptr[u]:test.indptr[u + 1]]
        assert np.array_equal(got0[b, :len(t)], pos0[b, t])
    with pytest.raises(IndexError):
        lg.rank_targets([0, U], test)
    assert lg.E0.weight.grad is None and lg.E0.weight.requires_grad


def test_get_metrics_at_equals_get_metrics_and_takes_k_above_1024():
    from gdmcf_amd.lightgcn import get_metrics, get_metrics_at
    rng = np.random.default_rng(5)
    U, I, d = 260, 1500, 16
    train, test = small_split(rng, U, I, 10, 5)
    ue = rng.integers(-3, 4, (U, d)).astype(np.float32)  # integer tables: the device ranking is the float64 ranking
    ie = rng.integers(-3, 4, (I, d)).astype(np.float32)
    ue_d, ie_d = torch.from_numpy(ue).to(DEV), torch.from_numpy(ie).to(DEV)
    at = get_metrics_at(ue_d, ie_d, U, I, train, test, [5, 20, 1100])
    assert list(at) == [5, 20, 1100]
    for K in (5, 20):
        assert at[K] == get_metrics(ue_d, ie_d, U, I, train, test, K), K  # the same hit matrix through the same arithmetic
    want = np_get_metrics(ue, ie, train, test, 1100)
    print("get_metrics_at[1100]", at[1100], "numpy", want)
    assert np.all(np.abs(np.asarray(at[1100]) - np.asarray(want)) <= 1e-12), (at[1100], want)
    assert at[1100][0] > at[20][0] > 0
    with pytest.raises(ValueError, match="1024"):
        get_metrics(ue_d, ie_d, U, I, train, test, 1100)  # (what get_metrics cannot take)


def test_rank_metrics_device_on_the_fused_ranks_equals_the_host_rank_metrics():
    rng = np.random.default_rng(9)
    U, I, d = 120, 700, 16
    train, test = small_split(rng, U, I, 10, 5)
    ue_d = torch.from_numpy(rng.integers(-3, 4, (U, d)).astype(np.float32)).to(DEV)
    ie_d = torch.from_numpy(rng.integers(-3, 4, (I, d)).astype(np.float32)).to(DEV)
    tp, tx = _t(test.indptr, torch.int64), _t(test.indices, torch.int32)
    ip, ix = _t(train.indptr, torch.int64), _t(train.indices, torch.int32)
    ranks = score_rank(ue_d, ie_d, tp, tx, ip, ix)
    topN = [1, 5, 20, 100, 1000]
    assert evaluate_utils.rank_metrics_device(ranks, topN) == evaluate_utils.rank_metrics(ranks.cpu().numpy(), topN)
    assert evaluate_utils.rank_metrics_device(ranks, topN)[1][-1] > 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_return_the_documented_codes_and_launch_nothing():
    lib = _lib.load()
    n_rows, I, d, G = 5, 40, 8, 3
    ue = torch.ones(n_rows, d, device=DEV)
    ie = torch.ones(I, d, device=DEV)
    tp = torch.arange(0, 2 * n_rows + 1, 2, dtype=torch.int64, device=DEV)
    tx = torch.zeros(2 * n_rows, dtype=torch.int32, device=DEV)
    out = torch.full((n_rows, G), FILL, dtype=torch.int32, device=DEV)
    nbytes = int(lib.gdmcf_score_rank_ws_bytes(n_rows, I, d, G))
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    assert lib.gdmcf_score_rank_ws_bytes(n_rows, I, d, 0) == 0

    def call(d_=d, G_=G, ip=None, ix=None, tp_=tp.data_ptr(), tx_=tx.data_ptr(), ws_=ws.data_ptr(), nb=nbytes, out_=out.data_ptr()):
        return lib.gdmcf_score_rank_f32(ue.data_ptr(), d, None, n_rows, ie.data_ptr(), d, I, d_, ip, ix, tp_, tx_, G_, out_, G, None,
                                        ws_, nb, _lib.stream_ptr())

    for code, kw in ((_lib.E_WORKSPACE, dict(nb=nbytes - 1)), (_lib.E_WORKSPACE, dict(ws_=None)), (_lib.E_SHAPE, dict(G_=0)),
                     (_lib.E_SHAPE, dict(d_=0)), (_lib.E_SHAPE, dict(G_=G + 1)), (_lib.E_ARG, dict(ip=tp.data_ptr())),
                     (_lib.E_ARG, dict(ix=tx.data_ptr())), (_lib.E_ARG, dict(tp_=None)), (_lib.E_ARG, dict(tx_=None)),
                     (_lib.E_ARG, dict(out_=None))):
        assert call(**kw) == code, kw
        assert b"score_rank" in lib.gdmcf_last_error()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((ws == 0x5A).all())  # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[:, :2] == 0).all()) and bool((out[:, 2] == -1).all())  # every score ties: two targets a row, item 0, rank 0
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.check(call(nb=8))
