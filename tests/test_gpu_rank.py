"""GPU: gdmcf_amd.rank_targets.  gdmcf_rank_targets_f32 against the positions in gdmcf_topk_masked_rows_f32's full
list (k = I), integer-exact, special values included; past the top-k's k against a numpy order; determinism and the columns it
must not write; gdmcf_rank_metrics_f64 against gdmcf_topn_metrics_f64, bit for bit; rank_targets against recommend(k = I) on every
route; chunks and ids; what is launched; driver.evaluate(recommend=True, ranks=True)."""
import ctypes
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib, driver, evaluate_utils
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import rank_targets, recommend
from tests import helpers as H
from tests.test_gpu_latent import _discrete, _fresh_dnn, _rows, cu, dnn_pair
from tests.test_gpu_recommend import (EMPTY, MESSY, N_USERS, SHORT, _case, _draws, _pred_in_wide_buffer, _raw_csr, _rows_call)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = -9  # what the output buffers hold before a launch


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def _csr_of(rows):
    """(indptr, indices) of hand-built rows: nothing is sorted, merged or range-checked."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate([np.asarray(r, dtype=np.int32) for r in rows] + [np.zeros(1, np.int32)])  # (never empty)


def _rank_call(pred, I, csr1, csr2, tgt, rows, G, pad=2, live=True):
    """(ranks [B, G + pad] pre-filled with FILL, n_live [B])"""
    B = pred.shape[0]
    out = torch.full((B, G + pad), FILL, dtype=torch.int32, device=DEV)
    n_live = torch.full((B,), FILL, dtype=torch.int32, device=DEV) if live else None
    ip1, ix1 = (_t(csr1[0], torch.int64), _t(csr1[1], torch.int32)) if csr1 is not None else (None, None)
    ip2, ix2 = (_t(csr2[0], torch.int64), _t(csr2[1], torch.int32)) if csr2 is not None else (None, None)
    tip, tix, rows_t = _t(tgt[0], torch.int64), _t(tgt[1], torch.int32), _t(rows, torch.int64)
    _lib.check(_lib.load().gdmcf_rank_targets_f32(
        pred.data_ptr(), pred.stride(0), B, I, _lib.ptr(ip1), _lib.ptr(ix1), _lib.ptr(ip2), _lib.ptr(ix2), tip.data_ptr(),
        tix.data_ptr(), _lib.ptr(rows_t), G, out.data_ptr(), out.stride(0), _lib.ptr(n_live), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), (n_live.cpu().numpy() if live else None)


def _expected(pos, tgt_rows, rows, I, G):
    """pos[b, item] = place of the item in the full list; -1 for targets out of range and for the columns past a row's length."""
    want = np.full((len(rows), G), -1, dtype=np.int64)
    for b, u in enumerate(rows):
        for j, t in enumerate(tgt_rows[u][:G]):
            if 0 <= t < I:
                want[b, j] = pos[b, t]
    return want


def _positions(idx):
    """idx [B, I]: a full list per row -> pos[b, item]"""
    idx = idx.cpu().numpy()
    assert (np.sort(idx, axis=1) == np.arange(idx.shape[1])).all()
    return np.argsort(idx, axis=1)


def _target_rows(I, mask_rows, seed):
    """The target rows of the N_USERS users: empty; one item; 70 items (more than a wave), unsorted, with a repeat; every item of
    the row; some masked items; -1 and I (out of range)."""
    rng = np.random.default_rng(seed)
    some = lambda n: rng.integers(0, I, n)
    seventy = rng.permutation(np.resize(rng.permutation(I), 69))
    seventy = np.append(seventy, seventy[3])  # a repeat
    t = [some(4) for _ in range(N_USERS)]
    t[0] = np.zeros(0, dtype=np.int64)
    t[1] = some(1)
    t[EMPTY] = seventy
    t[3] = np.arange(I)
    t[SHORT] = np.concatenate([mask_rows[SHORT][:4], some(3)])                    # masked ones first
    t[MESSY] = np.concatenate([[-1], mask_rows[MESSY][:3], [I], some(2), [I + 7]])  # masked and out of range
    t[8] = np.array([I, -1, 0, I - 1])
    return [np.asarray(r, dtype=np.int64) for r in t]


@pytest.mark.parametrize("I", [5, 131, 1030, 2048])
@pytest.mark.parametrize("B", [1, 7])
def test_kernel_gives_the_positions_of_the_full_top_k_list(I, B):
    k = min(3, I)  # (row SHORT leaves k - 1 items unmasked)
    ip1, ix1, rows1 = _raw_csr(I, k, 1)
    ip2, ix2, rows2 = _raw_csr(I, k, 2, special=False)
    tgt_rows = _target_rows(I, rows1, 5)
    tgt = _csr_of(tgt_rows)
    G = max(len(r) for r in tgt_rows)
    assert G == max(I, 70)
    picks = [[8, EMPTY, SHORT, EMPTY, 0, MESSY, 3]] if B == 7 else [[EMPTY], [SHORT], [MESSY], [3], [1]]  # unsorted, with a repeat
    in_range = lambda r: set(int(c) for c in r if 0 <= c < I)
    for rows in picks:
        rows = np.asarray(rows, dtype=np.int64)
        for ties in (True, False):
            pred = _pred_in_wide_buffer(B, I, 10 * I + int(ties), ties)
            assert pred.stride(0) == I + 13  # (rows that are only 4-byte aligned)
            for csr_a, csr_b in (((ip1, ix1), None), ((ip1, ix1), (ip2, ix2)), (None, None)):
                _, idx = _rows_call(pred, I, I, csr_a, csr_b, rows)  # the yardstick: the full list
                got, n_live = _rank_call(pred, I, csr_a, csr_b, tgt, rows, G)
                want = _expected(_positions(idx), tgt_rows, rows, I, G)
                assert np.array_equal(got[:, :G], want), (rows, ties, csr_b is not None)
                assert (got[:, G:] == FILL).all()
                masked = [(in_range(rows1[u]) if csr_a else set()) | (in_range(rows2[u]) if csr_b else set()) for u in rows]
                assert n_live.tolist() == [I - len(m) for m in masked]
        if EMPTY in rows:  # the row listed twice: both entries carry the one position
            b = list(rows).index(EMPTY)
            assert got[b, 69] == got[b, list(tgt_rows[EMPTY]).index(tgt_rows[EMPTY][69])] and got[b, 69] >= 0
    # rows == NULL: pred row b takes row b of every CSR; no n_live asked for
    pred = _pred_in_wide_buffer(B, I, 5, True)
    _, idx = _rows_call(pred, I, I, (ip1, ix1), None, None)
    got, _ = _rank_call(pred, I, (ip1, ix1), None, tgt, None, G, live=False)
    assert np.array_equal(got[:, :G], _expected(_positions(idx), tgt_rows, np.arange(B), I, G))


def test_special_values_order_as_in_the_top_k():
    I = 131
    g = torch.Generator().manual_seed(3)
    row = torch.randn(I, generator=g)
    neg_nan = torch.tensor([0xFFC00000 - (1 << 32)], dtype=torch.int32).view(torch.float32)[0]
    for at, v in ((3, float("nan")), (4, 0.0), (5, -0.0), (6, float("inf")), (7, float("-inf")), (60, float("nan")), (61, -0.0),
                  (62, 0.0), (63, float("-inf")), (64, float("inf")), (90, neg_nan), (91, float("-inf"))):
        row[at] = v
    buf = torch.full((2, I + 13), float("nan"))
    buf[0, :I], buf[1, :I] = row, row.flip(0)
    pred = cu(buf)[:, :I]
    mask_rows = [np.array([7, 20, 64]), np.array([], dtype=np.int64)]  # a masked -inf and a masked +inf among them
    mask = _csr_of(mask_rows)
    tgt_rows = [np.arange(I), np.arange(I)[::-1].copy()]
    _, idx = _rows_call(pred, I, I, mask, None, None)
    got, n_live = _rank_call(pred, I, mask, None, _csr_of(tgt_rows), None, I)
    assert np.array_equal(got[:, :I], _expected(_positions(idx), tgt_rows, [0, 1], I, I))
    assert n_live.tolist() == [I - 3, I]


@pytest.mark.parametrize("I", [4099, 40961])
def test_past_the_top_k_limit_against_a_numpy_order(I):
    """k = I is beyond gdmcf_topk_masked_rows_f32 here.  The oracle: a stable sort of -score with the masked items at -inf (inputs
    without NaN and -0.0, where numpy's order is the key order).  Row 0 names 1500 targets: more than one on-chip pass of 1024."""
    B = 3
    ip1, ix1, rows1 = _raw_csr(I, 20, 1)
    rows = np.asarray([MESSY, 0, SHORT], dtype=np.int64)
    g = torch.Generator().manual_seed(I)
    buf = torch.full((B, I + 13), float("nan"))
    buf[:, :I] = torch.round(torch.randn(B, I, generator=g) * 50) / 50 + 0.0  # ties; -0.0 + 0.0 = +0.0
    pred = cu(buf)[:, :I]
    host = buf[:, :I].numpy()
    assert not np.isnan(host).any() and not np.signbit(host[host == 0]).any()
    rng = np.random.default_rng(2)
    tgt_rows = [rng.integers(0, I, 10) for _ in range(N_USERS)]
    many = rng.permutation(I)[:1499]
    tgt_rows[MESSY] = np.append(many, many[7])                                        # 1500, unsorted, a repeat
    tgt_rows[SHORT] = np.concatenate([rows1[SHORT][:5], rng.integers(0, I, 5), [I, -1]])  # masked ones, out of range
    G = 1500
    got, n_live = _rank_call(pred, I, (ip1, ix1), None, _csr_of(tgt_rows), rows, G)
    pos = np.empty((B, I), dtype=np.int64)
    for b, u in enumerate(rows):
        s = host[b].copy()
        m = np.asarray([c for c in rows1[u] if 0 <= c < I], dtype=np.int64)
        s[m] = -np.inf
        pos[b, np.argsort(-s, kind="stable")] = np.arange(I)
        assert n_live[b] == I - len(set(m.tolist()))
    assert np.array_equal(got[:, :G], _expected(pos, tgt_rows, rows, I, G))
    assert (got[:, G:] == FILL).all()


def test_two_runs_give_equal_tensors():
    I, B = 4099, 7
    ip1, ix1, rows1 = _raw_csr(I, 20, 4)
    tgt_rows = _target_rows(I, rows1, 6)
    rows = np.asarray([8, EMPTY, SHORT, EMPTY, 0, MESSY, 3], dtype=np.int64)
    pred = _pred_in_wide_buffer(B, I, 9, True)  # ties: every gap counter is contended
    first = _rank_call(pred, I, (ip1, ix1), None, _csr_of(tgt_rows), rows, I, pad=5)
    again = _rank_call(pred, I, (ip1, ix1), None, _csr_of(tgt_rows), rows, I, pad=5)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    assert (first[0][:, I:] == FILL).all() and (first[0][:, :I] != FILL).all()
    # G below the longest row: the entries past G are not ranked, the columns past G not written
    short = _rank_call(pred, I, (ip1, ix1), None, _csr_of(tgt_rows), rows, 3, pad=5)[0]
    assert np.array_equal(short[:, :3], first[0][:, :3]) and (short[:, 3:] == FILL).all()


# ---------------------------------------------------------------------------------------------------------------------
# gdmcf_rank_metrics_f64
# ---------------------------------------------------------------------------------------------------------------------
def _topn_terms(order, truth, topN):
    """gdmcf_topn_metrics_f64's per-user terms [U, len(topN), 4] on the lists order[:, :max(topN)]"""
    U = order.shape[0]
    gt = _csr_of([sorted(t) for t in truth])
    out = torch.empty(U, len(topN), 4, dtype=torch.float64, device=DEV)
    ip, ix = _t(gt[0], torch.int64), _t(gt[1], torch.int32)
    _lib.check(_lib.load().gdmcf_topn_metrics_f64(order.data_ptr(), order.stride(0), U, ip.data_ptr(), ix.data_ptr(),
                                                  (ctypes.c_int * len(topN))(*topN), len(topN), out.data_ptr(), _lib.stream_ptr()))
    return out


def test_rank_metrics_carry_the_bits_of_topn_metrics():
    U, I = 40, 300
    rng = np.random.default_rng(11)
    truth = [rng.choice(I, size=int(n), replace=False).tolist() for n in np.resize(np.arange(26), U)]  # 0 .. 25 targets per user
    assert len(truth[0]) == 0 and max(len(t) for t in truth) == 25
    pred = _pred_in_wide_buffer(U, I, 2, True)
    _, order = _rows_call(pred, I, I, None, None, None)  # a full order per user
    G = 25
    ranks_np, _ = _rank_call(pred, I, None, None, _csr_of(truth), None, G, pad=0)
    assert np.array_equal(ranks_np, _expected(_positions(order), truth, np.arange(U), I, G))
    ranks = torch.from_numpy(ranks_np).to(DEV)
    topN = [1, 5, 20, 100, 300]
    got = evaluate_utils.rank_metrics_terms(ranks, topN)
    want = _topn_terms(order, truth, topN)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert float(want[:, :, 2].max()) > 0
    rounded = evaluate_utils.rank_metrics_device(ranks, topN)
    assert rounded == evaluate_utils.computeTopNAccuracy(truth, order.cpu().tolist(), topN)
    assert rounded == evaluate_utils.rank_metrics(ranks_np, topN)
    # a cut-off above the item count: every hit counts, recall is 1 for every user with targets
    has = torch.tensor([len(t) > 0 for t in truth], device=DEV)
    above = evaluate_utils.rank_metrics_terms(ranks, [300, 1000])
    assert torch.equal(above[:, 1, 1], has.double()) and torch.equal(above[:, 0].view(torch.int64), want[:, 4].view(torch.int64))
    # more cut-offs than one call takes: the host calls in groups, column for column the same bits
    many = [1, 2, 3, 5, 10, 20, 50, 100, 200, 300, 1000]
    grouped = evaluate_utils.rank_metrics_terms(ranks, many)
    for k, N in enumerate(many):
        assert torch.equal(grouped[:, k].view(torch.int64), evaluate_utils.rank_metrics_terms(ranks, [N])[:, 0].view(torch.int64))
    assert evaluate_utils.rank_metrics_device(ranks, many) == evaluate_utils.rank_metrics(ranks_np, many)


# ---------------------------------------------------------------------------------------------------------------------
# rank_targets end to end
# ---------------------------------------------------------------------------------------------------------------------
def _targets_like(dcsr, seed):
    a = (np.random.default_rng(seed).random(dcsr.shape) < 0.12).astype(np.float64)
    a[0] = 0  # a user without targets
    m = sp.csr_matrix(a)
    return m, DeviceCSR(m, DEV)


def _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt, **kw):
    I = dcsr.shape[1]
    assert I <= 2048
    idx = recommend(diff, model, dcsr, ids, I, return_values=False, **kw)
    route = diff.last_recommend_route
    diff.last_recommend_route = None
    ranks, live = rank_targets(diff, model, dcsr, ids, tgt, return_live=True, **kw)
    assert diff.last_recommend_route == route
    G = max(tgt.max_row_len, 1)
    assert ranks.dtype == torch.int32 and ranks.is_cuda and tuple(ranks.shape) == (len(ids), G)
    users = np.asarray(ids).tolist()
    tgt_rows = {u: tgt_host[u].indices for u in set(users)}
    assert np.array_equal(ranks.cpu().numpy(), _expected(_positions(idx), tgt_rows, users, I, G))
    assert bool((ranks >= 0).any())
    return route, ranks, live


@pytest.mark.parametrize("name", ["dnn_tiny", "onehot_tiny", "emb_tiny", "gcn_fresh"])
def test_rank_targets_equals_the_positions_in_recommends_full_list(monkeypatch, name):
    model, diff, x, ids, dcsr, _ = _case(name, monkeypatch)
    B, I = x.shape
    noise0, sampled0 = _draws(B, I)
    onehot = isinstance(diff, gdmcf_amd.GaussianDiffusionDiscrete)
    tgt_host, tgt = _targets_like(dcsr, 5)
    for steps, want_route in ((0, "latent-csr"), (diff.steps, "latent")):
        inj = {} if steps == 0 else (dict(noise0=noise0, sampled0=sampled0) if onehot else dict(noise0=noise0))
        route, ranks, live = _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt, sampling_steps=steps, **inj)
        assert route == want_route
        assert torch.equal(live.cpu(), torch.from_numpy(I - (x.numpy() != 0).sum(1)).to(torch.int32))  # mask="rows"
        assert torch.equal(rank_targets(diff, model, dcsr, ids, tgt, sampling_steps=steps, **inj), ranks)  # deterministic; ranks alone
    # another mask: None ranks the history too
    route, _, live = _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt, mask=None)
    assert route == "latent-csr" and bool((live == I).all())


def test_rank_targets_on_the_item_route_and_the_extended_routes():
    fx = H.load("sample_ragged_eps")  # the eps target: "item" with latent=True, the bracket ranking with latent="extended"
    model, diff = dnn_pair(H.sample_meta(fx), fx)
    x = fx["x_start"].astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(x.astype(np.float64)), DEV)
    ids = np.arange(x.shape[0])
    tgt_host, tgt = _targets_like(dcsr, 6)
    assert _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt)[0] == "item"
    assert _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt, latent="extended", mask="rows")[0] == "latent-csr"
    assert _check_against_full_lists(diff, model, dcsr, ids, tgt_host, tgt, latent="extended", mask=None)[0] == "latent"
    fx = H.load("dnncat_sample_tiny_x0")  # DNNCat
    meta = H.onehot_sample_meta(fx)
    I, dims = meta["I"], meta["dims"]
    cat = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], 10)
    cat.load_state_dict(H.state_dict_from(fx))
    cat, diff = cat.to(DEV).eval(), _discrete(meta)
    x = fx["x_start"].astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(x.astype(np.float64)), DEV)
    tgt_host, tgt = _targets_like(dcsr, 7)
    ids = np.arange(x.shape[0])
    assert _check_against_full_lists(diff, cat, dcsr, ids, tgt_host, tgt)[0] == "item"
    assert _check_against_full_lists(diff, cat, dcsr, ids, tgt_host, tgt, latent="extended")[0] == "latent-csr"


def test_chunks_permutations_and_repeats():
    I, U = 131, 10
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    _, tgt = _targets_like(dcsr, 8)
    ids = torch.arange(U)
    ranks, live = rank_targets(diff, model, dcsr, ids, tgt, return_live=True)  # one chunk
    r3, l3 = rank_targets(diff, model, dcsr, ids, tgt, batch_size=3, return_live=True)
    assert torch.equal(r3, ranks) and torch.equal(l3, live)
    assert bool((ranks[0] == -1).all()) and bool((ranks >= 0).any())
    perm = [7, 2, 9, 2, 0, 5, 1, 8, 3, 6, 4]  # a permutation with a repeat: rows follow their ids
    rp, lp = rank_targets(diff, model, dcsr, perm, tgt, batch_size=3, return_live=True)
    sel = torch.tensor(perm, device=DEV)
    assert torch.equal(rp, ranks[sel]) and torch.equal(lp, live[sel])
    assert torch.equal(rank_targets(diff, model, dcsr, cu(torch.tensor(perm)), tgt), ranks[sel])  # ids already on the device
    with pytest.raises(IndexError):
        rank_targets(diff, model, dcsr, [0, U], tgt)
    assert rank_targets(diff, model, dcsr, [], tgt).shape == (0, tgt.max_row_len)
    empty = DeviceCSR(sp.csr_matrix((U, I)), DEV)  # no target at all: one column of -1
    none = rank_targets(diff, model, dcsr, ids, empty)
    assert tuple(none.shape) == (U, 1) and bool((none == -1).all())


def test_one_rank_launch_per_chunk_no_top_k_and_no_synchronisation_between_chunks(monkeypatch):
    I, U, bs = 131, 10, 4
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    _, tgt = _targets_like(dcsr, 8)
    want = rank_targets(diff, model, dcsr, np.arange(U), tgt, batch_size=bs)  # builds the cached operands
    lib = _lib.load()
    calls, seen = [], []
    for name in ("gdmcf_rank_targets_f32", "gdmcf_topk_masked_rows_f32", "gdmcf_topk_masked_f32", "gdmcf_score_topk_f32"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda nm, fn: lambda *a: (calls.append((nm, a, len(seen))), fn(*a))[1])(name, real),
                            raising=False)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:  # (every synchronising torch call leaves one warning here)
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            got = rank_targets(diff, model, dcsr, np.arange(U), tgt, batch_size=bs)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert diff.last_recommend_route == "latent-csr"
    assert [c[0] for c in calls] == ["gdmcf_rank_targets_f32"] * 3
    assert [c[1][2] for c in calls] == [4, 4, 2] and all(c[1][3] == I and c[1][11] == tgt.max_row_len for c in calls)  # B, I, G
    assert calls[0][2] == calls[-1][2] == len(seen), [str(w.message) for w in seen]  # nothing synchronised from the first launch on
    assert torch.equal(got, want)


@pytest.mark.parametrize("backbone", ["dnn", "emb"])
def test_evaluate_with_ranks_gives_the_lists_metrics(backbone):
    U, I, bs, topN = 37, 131, 8, [1, 5, 10, 50]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    if backbone == "dnn":
        model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=2)
    else:
        torch.manual_seed(2)
        model = gdmcf_amd.DNNOneHotEmbedding([I, 24], [24, I], 10, item_num=I, user_num=U).to(DEV).eval()
        diff = _discrete(dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=5, discrete=0.99), index_in=True)
    want = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True)
    got = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True, ranks=True)
    assert got == want, (got, want)
    assert max(want[1]) > 0
    # no list bounds the cut-offs any more: N above the item count
    wide = driver.evaluate(diff, model, train, test, train, [5, 10, 1000], 0, False, bs, DEV, recommend=True, ranks=True)
    assert [wide[m][:2] for m in range(4)] == [want[m][1:3] for m in range(4)]
    assert wide[1][2] == round(int((np.diff(test.indptr) > 0).sum()) / U, 4)
    with pytest.raises(ValueError, match="ranks"):
        driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, ranks=True)
    with pytest.raises(ValueError, match="ranks"):
        driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True, ranks=True,
                        candidates=np.zeros((U, 8), dtype=np.int64))
