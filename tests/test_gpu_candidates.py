"""GPU: candidate lists.  gdmcf_cand_scores_f32 against float64 under a derived bound on aligned and on unaligned
operands, its bits against the candidate's place in the list, its masks against a numpy membership test on raw CSRs;
gdmcf_cand_pick_f32 bit for bit; recommend(candidates=) against recommend() and against the float64 oracle restricted to the
lists on both routes; score_candidates; the launches of the "gathered" route; the "auto" rule; freshness after an optimiser
step; LightGCN.recommend's lists handed on; driver.evaluate(candidates=)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib, driver, evaluate_utils
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import recommend, score_candidates
from tests import helpers as H
from tests.test_gpu_latent import _fresh_dnn, _oracle64, _rows, cu, dnn_pair
from tests.test_gpu_latent_ext import _rec_case
from tests.test_gpu_recommend import EMPTY, MESSY, N_USERS, SHORT, _case, _check_lists, _draws, _raw_csr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
def _seat(data, odd):
    """`data` [R, n] on the device: odd -- inside a NaN-filled buffer with an odd row stride above n and an odd element offset
    (rows 4-byte aligned only); otherwise with a row stride that is a multiple of four elements (rows 16-byte aligned)."""
    R, n = data.shape
    ld = (n + 3) | 1 if odd else (n + 3) // 4 * 4
    buf = torch.full((R * ld + 1,), float("nan"), device=DEV)
    view = torch.as_strided(buf, (R, n), (ld, 1), 1 if odd else 0)
    view.copy_(data)
    assert (view.data_ptr() % 16 == 0 and ld % 4 == 0) != odd
    return buf, view


def _dev(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def _masks(csr1, csr2, rows):
    ip1, ix1 = (_dev(csr1[0], torch.int64), _dev(csr1[1], torch.int32)) if csr1 is not None else (None, None)
    ip2, ix2 = (_dev(csr2[0], torch.int64), _dev(csr2[1], torch.int32)) if csr2 is not None else (None, None)
    return (ip1, ix1, ip2, ix2), _dev(rows, torch.int64)


def _scores_call(A, W, I, K, bias, scale, cand, csr1=None, csr2=None, rows=None, odd_out=False):
    """gdmcf_cand_scores_f32 into a NaN-filled buffer; cand [B, C] or a shared [C] (ldcand = 0)."""
    B = A.shape[0]
    C = cand.shape[-1]
    obuf, out = _seat(torch.full((B, C), float("nan")), odd_out)
    keep, rows_t = _masks(csr1, csr2, rows)
    core.cand_scores(_lib.load(), A, W, I, K, bias, scale, cand, 0 if cand.dim() == 1 else cand.stride(0), B, C,
                     tuple(_lib.ptr(t) for t in keep), rows_t, out, _lib.stream_ptr())
    torch.cuda.synchronize()
    inside = torch.zeros(obuf.numel(), dtype=torch.bool, device=DEV)
    torch.as_strided(inside, out.shape, out.stride(), out.storage_offset()).fill_(True)
    assert bool(torch.isnan(obuf[~inside]).all()), "a store outside out[B, C]"
    return out.clone()


_OPERANDS = {}


def _operands(B, I, K):
    """Shared among the cases: A [B, K], W [I, K], bias [I], scale [B] (host, float32)."""
    key = (B, I, K)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(1000 * B + K)
        _OPERANDS[key] = (torch.randn(B, K, generator=g), torch.randn(I, K, generator=g), torch.randn(I, generator=g),
                          torch.rand(B, generator=g) + 0.5)
    return _OPERANDS[key]


I_KERNEL = 97
KERNEL_CASES = [(K, 7, 65) for K in (1, 3, 4, 255, 256, 260, 1000, 3000, 4096)] + \
               [(260, B, C) for C in (1, 3, 64, 65, 130) for B in (1, 7)]


@pytest.mark.parametrize("K,B,C", KERNEL_CASES)
def test_gathered_product_matches_float64(K, B, C):
    """Bound, derived: K fused multiply-adds (exact products, one rounding each) and the additions of the butterfly come to at
    most K roundings on the way to a sum of K products, the bias adds one and the scale one -- (K + 2) roundings of relative
    size 2^-24, each of a partial result no larger than sum |a w| + |bias|, times |scale|; 1.01 covers the second-order terms."""
    I = I_KERNEL
    A, W, bias, scale = _operands(B, I, K)
    cand = torch.randint(0, I, (B, C), generator=torch.Generator().manual_seed(C + K))
    got_c = cand.numpy()
    dot = np.einsum("bk,bck->bc", A.double().numpy(), W.double().numpy()[got_c])
    mag = np.einsum("bk,bck->bc", A.double().abs().numpy(), W.double().abs().numpy()[got_c])
    ref = (dot + bias.double().numpy()[got_c]) * scale.double().numpy()[:, None]
    bound = 1.01 * (K + 2) * 2.0 ** -24 * np.abs(scale.double().numpy())[:, None] * (mag + np.abs(bias.double().numpy()[got_c]))
    worst = 0.0
    for odd in (False, True):
        (_, a), (_, w) = _seat(A, odd), _seat(W, odd)
        assert a.stride(0) >= K and w.stride(0) >= K and (not odd or (a.stride(0) > K and w.stride(0) > K))
        out = _scores_call(a, w, I, K, cu(bias), cu(scale), cu(cand), odd_out=odd)
        assert not bool(torch.isnan(out).any()), "padding was read"
        err = np.abs(out.cpu().double().numpy() - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (K, B, C, odd, float((err / bound).max()))
    print(f"K={K} B={B} C={C}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("K", [0, 4097])
def test_gathered_product_refuses_k_outside_its_limits(K):
    A, W, bias, scale = (cu(t) for t in _operands(7, I_KERNEL, 260))
    cand = cu(torch.zeros(7, 3, dtype=torch.int64))
    out = cu(torch.zeros(7, 3))
    lib = _lib.load()
    rc = lib.gdmcf_cand_scores_f32(A.data_ptr(), 4100, W.data_ptr(), 4100, I_KERNEL, K, None, None, cand.data_ptr(), 3, 7, 3,
                                   None, None, None, None, None, out.data_ptr(), 3, _lib.stream_ptr())
    assert rc == _lib.E_SHAPE and b"gdmcf_cand_scores_f32" in lib.gdmcf_last_error()
    assert not bool(out.any())


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("with_bias_scale", [True, False])
def test_bits_do_not_depend_on_the_place_in_the_list(with_bias_scale):
    B, I, K, C = 5, 64, 260, 23
    A, W, bias, scale = (cu(t) for t in _operands(B, I, K))
    if not with_bias_scale:
        bias = scale = None
    full = _scores_call(A, W, I, K, bias, scale, cu(torch.arange(I)))  # every item, one shared list: the table of (b, item)
    assert bool(torch.isfinite(full).all())
    g = torch.Generator().manual_seed(3)
    lists = torch.stack([torch.randperm(I, generator=g)[:C] for _ in range(B)])
    want = lambda cand: torch.gather(full, 1, cu(cand))

    def same(cand, out):
        assert torch.equal(_bits(out), _bits(want(cand)))

    same(lists, _scores_call(A, W, I, K, bias, scale, cu(lists)))
    same(lists, _scores_call(A, W, I, K, bias, scale, cu(lists)))  # run twice
    perm = torch.stack([row[torch.randperm(C, generator=g)] for row in lists])
    same(perm, _scores_call(A, W, I, K, bias, scale, cu(perm)))
    for lo, hi in ((0, 10), (10, C)):  # split in two calls (views: ldcand above the call's C)
        view = cu(lists)[:, lo:hi]
        assert view.stride(0) == C
        same(lists[:, lo:hi], _scores_call(A, W, I, K, bias, scale, view))
    shared = lists[2]
    rep = shared.expand(B, C).contiguous()
    out_shared = _scores_call(A, W, I, K, bias, scale, cu(shared))
    same(rep, out_shared)
    assert torch.equal(_bits(out_shared), _bits(_scores_call(A, W, I, K, bias, scale, cu(rep))))
    dup = torch.cat([lists, lists[:, :4]], dim=1)  # duplicates are each scored
    same(dup, _scores_call(A, W, I, K, bias, scale, cu(dup)))


ROW_PICKS = [np.asarray([8, EMPTY, SHORT, EMPTY, 0, MESSY, 3], dtype=np.int64), None]


def _mask_case(I, C, seed):
    """(csr1, csr2, per-row index arrays of both, candidates [B, C] with -1, I, 2**40 and a duplicate in every list)"""
    ip1, ix1, rows1 = _raw_csr(I, 1, seed)  # (k = 1: row SHORT masks every item, so every candidate)
    ip2, ix2, rows2 = _raw_csr(I, 1, seed + 1, special=False)
    ix2 = ix2.copy()
    ix2[::7] = np.where(np.arange(len(ix2[::7])) % 2 == 0, -5, I + 7)  # out-of-range entries mask nothing
    rows2 = [ix2[ip2[u]:ip2[u + 1]] for u in range(N_USERS)]
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, I, (7, C), generator=g)
    cand[:, 1], cand[:, 4], cand[:, C - 1] = -1, I, 2 ** 40
    cand[:, 5] = cand[:, 2]
    return (ip1, ix1), (ip2, ix2), rows1, rows2, cand


def _membership(cand, I, rows, *row_sets):
    c = cand.numpy()
    dead = (c < 0) | (c >= I)
    for b in range(c.shape[0]):
        r = b if rows is None else int(rows[b])
        for rs in row_sets:
            dead[b] |= np.isin(c[b], rs[r])
    return torch.from_numpy(dead)


@pytest.mark.parametrize("C", [9, 70])
def test_masks_match_a_membership_test_on_raw_csrs(C):
    I, K, B = 131, 260, 7
    A, W, bias, scale = (cu(t) for t in _operands(B, I, K))
    csr1, csr2, rows1, rows2, cand = _mask_case(I, C, 5)
    safe = cand.clamp(0, I - 1)
    free = torch.gather(_scores_call(A, W, I, K, bias, scale, cu(torch.arange(I))), 1, cu(safe))
    for rows in ROW_PICKS:
        for second in (None, csr2):
            dead = _membership(cand, I, rows, rows1, *(() if second is None else (rows2,)))
            if rows is not None:
                assert bool(dead[2].all()), "row SHORT masks every candidate"
            assert bool((~dead).any())
            want = torch.where(cu(dead), torch.full_like(free, NEG_INF), free)
            out = _scores_call(A, W, I, K, bias, scale, cu(cand), csr1, second, rows)
            assert torch.equal(_bits(out), _bits(want)), (C, rows is None, second is not None)
    dead = _membership(cand, I, None)  # no mask: only the candidates outside [0, I)
    out = _scores_call(A, W, I, K, bias, scale, cu(cand))
    assert torch.equal(_bits(out), _bits(torch.where(cu(dead), torch.full_like(free, NEG_INF), free)))
    assert int(dead.sum()) == 3 * B


# ---- runs longer than one group of four: a wave takes S list positions, S from B * C (cand_scores.hip: cs_run_length) ---------------
def _run_length(B, C):
    """cs_run_length restated: the smallest multiple of four that puts 4 096 waves on the chip, between 4 and 64."""
    s = -(-(B * C) // 4096)
    return min(max(-(-s // 4) * 4, 4), 64)


def _long_lists(B, C, I, seed):
    """Candidates with dead ones spread through every run: about one in ten outside [0, I) (-1, -3, I, I + 2, 2**40), the rest
    random items, of which the mask rows remove more; the first run of row 0 is all dead, the second has one live candidate."""
    g = torch.Generator().manual_seed(seed)
    cand = torch.randint(0, I, (B, C), generator=g)
    bad = torch.tensor([-1, -3, I, I + 2, 2 ** 40])
    hole = torch.rand(B, C, generator=g) < 0.1
    cand[hole] = bad[torch.randint(0, len(bad), (int(hole.sum()),), generator=g)]
    S = _run_length(B, C)
    cand[0, :2 * S] = -1
    cand[0, S + S // 2] = 5
    return cand


LONG_RUNS = [(4, 64, 300, 8), (260, 7, 10000, 20), (4, 5, 52000, 64), (1000, 3, 6001, 8)]


@pytest.mark.parametrize("K,B,C,S", LONG_RUNS)
def test_gathered_product_with_runs_of_several_groups(K, B, C, S):
    """The shapes above are tiny in work but large in B * C, so that a wave's run holds 2, 5 and 16 groups of four (and, with C no
    multiple of S, a shorter last run): the group loop's later passes, a partial last group behind full ones, dead candidates in
    the middle of a run, whole runs without a live candidate, runs that start at S * segment.  Live scores against float64 under
    test_gathered_product_matches_float64's bound, dead ones -inf, on aligned and on unaligned operands."""
    assert _run_length(B, C) == S and C > S
    I = I_KERNEL
    A, W, bias, scale = _operands(B, I, K)
    csr1, csr2, rows1, rows2, _ = _mask_case(I, 9, 5)
    rows = np.arange(B, dtype=np.int64)[::-1] % N_USERS  # unsorted, with repeats
    cand = _long_lists(B, C, I, K + C)
    dead = _membership(cand, I, rows, rows1, rows2)
    assert bool(dead[0, :S].all()) and int((~dead).sum()) > B * C // 4 and bool(dead[:, S:].any())
    idx = cand.clamp(0, I - 1).numpy()
    a64, w64, b64, s64 = (t.double().numpy() for t in (A, W, bias, scale))
    dot, mag = np.take_along_axis(a64 @ w64.T, idx, 1), np.take_along_axis(np.abs(a64) @ np.abs(w64).T, idx, 1)
    ref = (dot + b64[idx]) * s64[:, None]
    bound = 1.01 * (K + 2) * 2.0 ** -24 * np.abs(s64)[:, None] * (mag + np.abs(b64[idx]))
    live = ~dead.numpy()
    worst = 0.0
    for odd in (False, True):
        (_, a), (_, w) = _seat(A, odd), _seat(W, odd)
        out = _scores_call(a, w, I, K, cu(bias), cu(scale), cu(cand), csr1, csr2, rows, odd_out=odd).cpu()
        assert not bool(torch.isnan(out).any()), "padding was read"
        assert torch.equal(torch.isneginf(out), dead), "dead candidates, and only they, carry -inf"
        err = np.abs(out.double().numpy() - ref)[live]
        worst = max(worst, float((err / bound[live]).max()))
        assert (err <= bound[live]).all(), (K, B, C, odd, worst)
    print(f"K={K} B={B} C={C} S={S}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("C,S", [(4000, 8), (16500, 24), (52000, 64)])
def test_bits_do_not_depend_on_the_run_length(C, S):
    """The table of (b, item) built by a call whose runs are one group of four, against calls whose runs are S = 8, 24 and 64
    positions long -- other C, other run length, other segment starts, the same bits; masked and out-of-range candidates -inf."""
    B, I, K = 5, 64, 260
    assert _run_length(B, I) == 4 and _run_length(B, C) == S
    A, W, bias, scale = (cu(t) for t in _operands(B, I, K))
    full = _scores_call(A, W, I, K, bias, scale, cu(torch.arange(I)))
    csr1, _, rows1, _, _ = _mask_case(I, 9, 5)
    rows = np.asarray([8, EMPTY, MESSY, 0, 3], dtype=np.int64)
    cand = _long_lists(B, C, I, C)
    dead = _membership(cand, I, rows, rows1)
    assert bool((~dead).any(dim=1).all())
    want = torch.where(cu(dead), torch.full_like(full[:, :1], NEG_INF).expand(B, C), torch.gather(full, 1, cu(cand.clamp(0, I - 1))))
    out = _scores_call(A, W, I, K, bias, scale, cu(cand), csr1, None, rows)
    assert torch.equal(_bits(out), _bits(want))
    shared = cu(cand[1].contiguous())  # one shared list, no mask
    dead = _membership(cand[1].expand(B, C), I, None)
    want = torch.where(cu(dead), torch.full_like(full[:, :1], NEG_INF).expand(B, C),
                       torch.gather(full, 1, shared.clamp(0, I - 1).expand(B, C)))
    assert torch.equal(_bits(_scores_call(A, W, I, K, bias, scale, shared)), _bits(want))


@pytest.mark.parametrize("C", [9, 70])
def test_pick_matches_where_bit_for_bit(C):
    I, B = 131, 7
    g = torch.Generator().manual_seed(8)
    buf = torch.full((B, I + 13), float("nan"))
    buf[:, :I] = torch.randn(B, I, generator=g)
    dense = cu(buf)[:, :I]
    assert dense.stride(0) > I
    scale = cu(torch.rand(B, generator=g) + 0.5)
    csr1, csr2, rows1, rows2, cand = _mask_case(I, C, 9)
    picked = torch.gather(dense, 1, cu(cand.clamp(0, I - 1)))
    lib = _lib.load()
    for rows in ROW_PICKS:
        for second in (None, csr2):
            for sc in (scale, None):
                dead = _membership(cand, I, rows, rows1, *(() if second is None else (rows2,)))
                live = picked * sc[:, None] if sc is not None else picked
                want = torch.where(cu(dead), torch.full_like(live, NEG_INF), live)
                keep, rows_t = _masks(csr1, second, rows)
                obuf, out = _seat(torch.full((B, C), float("nan")), True)
                core.cand_pick(lib, dense, B, I, sc, cu(cand), C, C, tuple(_lib.ptr(t) for t in keep), rows_t, out, _lib.stream_ptr())
                torch.cuda.synchronize()
                assert torch.equal(_bits(out), _bits(want)), (C, rows is None, second is not None, sc is not None)
    shared = cu(cand[0].contiguous())  # ldcand = 0
    out = cu(torch.full((B, C), float("nan")))
    core.cand_pick(lib, dense, B, I, None, shared, 0, C, (None,) * 4, None, out, _lib.stream_ptr())
    dead = _membership(cand[0].expand(B, C), I, None)
    want = torch.where(cu(dead), torch.full_like(out, NEG_INF), torch.gather(dense, 1, shared.clamp(0, I - 1).expand(B, C)))
    assert torch.equal(_bits(out), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# through recommend / score_candidates
# ---------------------------------------------------------------------------------------------------------------------
def _norm_case():
    fx = H.load("sample_norm_x0")
    model, diff = dnn_pair(H.sample_meta(fx), fx)
    x = torch.from_numpy(fx["x_start"].astype(np.float32))
    return model, diff, x, torch.arange(x.shape[0]), DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)


@pytest.mark.parametrize("name", ["dnn_deep", "onehot_tiny", "emb_tiny", "gcn_fresh", "item_norm"])
def test_every_item_as_candidates_picked_equals_recommend(monkeypatch, name):
    """candidates = arange(I): positions are item ids, so the tie rules coincide."""
    if name == "item_norm":
        model, diff, x, ids, dcsr = _norm_case()
    else:
        model, diff, x, ids, dcsr, _ = _case(name, monkeypatch)
    I = x.shape[1]
    for k in (1, 20):
        want = recommend(diff, model, dcsr, ids, k, return_values=True)
        route = diff.last_recommend_route
        assert route == ("item" if name == "item_norm" else "latent-csr")
        for cand in (torch.arange(I), torch.arange(I).expand(len(ids), I)):
            val, idx = recommend(diff, model, dcsr, ids, k, return_values=True, candidates=cand, candidate_route="picked")
            assert diff.last_candidate_route == "picked" and diff.last_recommend_route == route
            assert torch.equal(idx, want[1]) and torch.equal(_bits(val), _bits(want[0]))


def _lists(x, C, seed):
    """Unique items per user; the list of the user with the longest history (_heavy) starts with that history, so that it holds
    more masked candidates than C - k for the k in use (all of them where the history is long enough)."""
    B, I = x.shape
    rng = np.random.default_rng(seed)
    out = np.stack([rng.permutation(I)[:C] for _ in range(B)])
    u = _heavy(x)
    his = np.flatnonzero(x[u].numpy() != 0)
    rest = np.setdiff1d(np.arange(I), his)
    out[u] = np.concatenate([rng.permutation(his), rng.permutation(rest)])[:C]
    return torch.from_numpy(out)


def _heavy(x):
    return int((x != 0).sum(dim=1).argmax())


def _positions(idx, cand):
    """Item ids [n, k] -> positions in the user's (duplicate-free) list."""
    hit = idx.cpu()[:, :, None] == cand[:, None, :]
    assert bool((hit.sum(dim=2) == 1).all()), "an id that is not in the user's list"
    return hit.long().argmax(dim=2)


ORACLE_CASES = [("dnn_deep", True), ("onehot_tiny", True), ("emb_tiny", True), ("gcn_fresh", True), ("dnn_eps", "extended"),
                ("cat_x0", "extended")]


@pytest.mark.parametrize("name,latent", ORACLE_CASES)
def test_candidate_lists_match_the_float64_oracle(monkeypatch, name, latent):
    if latent is True:
        model, diff, x, ids, dcsr, ref_of = _case(name, monkeypatch)
    else:
        model, diff, x, ref_of = _rec_case(name, monkeypatch)
        ids, dcsr = torch.arange(x.shape[0]), DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    B, I = x.shape
    noise0, sampled0 = _draws(B, I)
    onehot = isinstance(diff, gdmcf_amd.GaussianDiffusionDiscrete)
    masked = x.numpy() != 0
    worst = {}
    for steps in (0, diff.steps):
        inj = {} if steps == 0 else (dict(noise0=noise0, sampled0=sampled0) if onehot else dict(noise0=noise0))
        ref = ref_of(steps, inj.get("noise0"), inj.get("sampled0"))
        product = not (name == "dnn_eps" and steps > 0)  # the EPSILON target on dense rows ends in the posterior epilogue
        for C in (5, 40):
            assert C <= I
            cand = _lists(x, C, 10 * C + steps)
            ref_c, own = np.take_along_axis(ref, cand.numpy(), 1), np.take_along_axis(masked, cand.numpy(), 1)
            # k = 1 needs every candidate of one user masked to have more masked ones than C - k: a second mask matrix that
            # lists the heavy user's whole list (k = C: the history at the head of that list is enough)
            u = _heavy(x)
            extra = DeviceCSR(sp.csr_matrix((np.ones(C), (np.full(C, int(ids[u])), cand[u].numpy())), shape=tuple(dcsr.shape)), DEV)
            whole = own.copy()
            whole[u] = True
            for route in ("gathered", "picked"):
                for k in (1, C):
                    masked_c, mask = (whole, (dcsr, extra)) if k == 1 else (own, "rows")
                    kw = dict(sampling_steps=steps, return_values=True, latent=latent, candidates=cand, candidate_route=route,
                              mask=mask, **inj)
                    if route == "gathered" and not product:
                        with pytest.raises(ValueError, match="gathered"):
                            recommend(diff, model, dcsr, ids, k, **kw)
                        continue
                    assert masked_c[u].sum() > C - k
                    val, idx = recommend(diff, model, dcsr, ids, k, **kw)
                    assert diff.last_candidate_route == route
                    assert idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
                    what = f"{name} steps={steps} C={C} {route} k={k}"
                    _check_lists(val, _positions(idx, cand), ref_c, masked_c, k, what)
                    fin = torch.isfinite(val).cpu().numpy()
                    dev = np.abs(val.cpu().double().numpy() - np.take_along_axis(ref_c, _positions(idx, cand).numpy(), 1))[fin]
                    worst[route] = max(worst.get(route, 0.0), float(dev.max(initial=0.0)))
    print(f"{name}: worst value deviation {worst}")


def test_score_candidates_shared_lists_masks_and_chunks():
    I, U, C = 131, 10, 20
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    x = _rows(U, I, 7)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    ids = [3, 3, 9, 0, 3, 7, 1, 9]
    shared = torch.from_numpy(np.random.default_rng(1).permutation(I)[:C])
    masked = torch.gather(x[ids] != 0, 1, shared.expand(len(ids), C))
    assert bool(masked.any()) and not bool(masked.all())
    for route in ("gathered", "picked"):
        one = score_candidates(diff, model, dcsr, ids, shared, candidate_route=route)
        assert one.shape == (len(ids), C) and one.dtype == torch.float32 and one.is_cuda
        assert diff.last_candidate_route == route and diff.last_recommend_route == "latent-csr"
        assert torch.equal(torch.isneginf(one).cpu(), masked) and bool(torch.isfinite(one).cpu()[~masked].all())
        rep = score_candidates(diff, model, dcsr, ids, shared.expand(len(ids), C), candidate_route=route)
        assert torch.equal(_bits(rep), _bits(one))
        chunked = score_candidates(diff, model, dcsr, ids, shared.expand(len(ids), C), candidate_route=route, batch_size=3)
        assert torch.equal(_bits(chunked), _bits(one))
        assert torch.equal(_bits(score_candidates(diff, model, dcsr, ids, shared, candidate_route=route, batch_size=3)), _bits(one))
        free = score_candidates(diff, model, dcsr, ids, shared, mask=None, candidate_route=route)
        assert bool(torch.isfinite(free).all()) and torch.equal(_bits(free).cpu()[~masked], _bits(one).cpu()[~masked])
    assert score_candidates(diff, model, dcsr, [], shared).shape == (0, C)


def _count_calls(monkeypatch, lib, names):
    """Counts C-ABI calls by entry point: (name, args) per call."""
    calls = []
    for name in names:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda nm, fn: lambda *a: (calls.append((nm, a)), fn(*a))[1])(name, real), raising=False)
    return calls


def test_gathered_route_launches(monkeypatch):
    I, U, bs, C, k = 131, 10, 4, 20, 5
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    cand = _lists(_rows(U, I, 7), C, 2)
    recommend(diff, model, dcsr, np.arange(U), k, batch_size=bs)  # builds the cached operands (their own item-wide product)
    calls = _count_calls(monkeypatch, _lib.load(), [
        "gdmcf_linear_fwd_f32", "gdmcf_linear_fwd_wt_f32", "gdmcf_linear_posterior_fwd_f32", "gdmcf_topk_masked_rows_f32",
        "gdmcf_topk_masked_f32", "gdmcf_cand_scores_f32", "gdmcf_cand_pick_f32"])
    recommend(diff, model, dcsr, np.arange(U), k, batch_size=bs, candidates=cand, candidate_route="gathered")
    assert diff.last_candidate_route == "gathered" and diff.last_recommend_route == "latent-csr"
    n_batches = -(-U // bs)
    names = [c[0] for c in calls]
    # gdmcf_linear_fwd*_f32: ..., act, M, N, K at positions 6, 7, 8
    assert not [c for c in calls if c[0].startswith("gdmcf_linear_fwd") and c[1][7] == I], "an item-wide product"
    assert "gdmcf_linear_posterior_fwd_f32" not in names and "gdmcf_topk_masked_rows_f32" not in names
    assert "gdmcf_cand_pick_f32" not in names
    assert names.count("gdmcf_cand_scores_f32") == n_batches
    topk = [c for c in calls if c[0] == "gdmcf_topk_masked_f32"]
    assert [c[1][3] for c in topk] == [C] * n_batches and [c[1][2] for c in topk] == [4, 4, 2]
    # "picked" on the same call: the item-wide product and one pick per chunk instead
    del calls[:]
    recommend(diff, model, dcsr, np.arange(U), k, batch_size=bs, candidates=cand, candidate_route="picked")
    names = [c[0] for c in calls]
    assert len([c for c in calls if c[0].startswith("gdmcf_linear_fwd") and c[1][7] == I]) == n_batches
    assert names.count("gdmcf_cand_pick_f32") == n_batches and "gdmcf_cand_scores_f32" not in names


def test_auto_follows_the_rule_and_gathered_needs_a_product():
    I, U, C = 131, 10, 20
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    shared = torch.arange(C)
    recommend(diff, model, dcsr, [0, 1], 5, candidates=shared)
    assert diff.last_candidate_route == "gathered"  # 2 x 20 <= 131
    recommend(diff, model, dcsr, np.arange(7), 5, candidates=shared)
    assert diff.last_candidate_route == "picked"    # 7 x 20 > 131
    recommend(diff, model, dcsr, np.arange(7), 5, candidates=shared, batch_size=4)
    assert diff.last_candidate_route == "gathered"  # the rule is per chunk: the last one has 3 users
    with pytest.raises(ValueError, match="gathered"):  # sampling noise: the "item" route
        recommend(diff, model, dcsr, [0, 1], 5, candidates=shared, sampling_noise=True, candidate_route="gathered")
    assert diff.last_recommend_route == "item"
    score_candidates(diff, model, dcsr, [0, 1], shared, sampling_noise=True)
    assert diff.last_candidate_route == "picked"


def test_gathered_scores_follow_an_eager_optimiser_step(monkeypatch):
    I, B, C = 131, 10, 12
    model, diff, meta = _fresh_dnn(I, [24], [24], 5, seed=4)
    x = _rows(B, I, 6)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    cand = _lists(x, C, 3)
    ids = np.arange(B)
    before = score_candidates(diff, model, dcsr, ids, cand, mask=None, candidate_route="gathered")
    opt = torch.optim.Adam(model.parameters(), lr=0.02)  # (every weight moves by about lr, whatever the gradient's scale)
    model.train()
    model.drop.p = 0.0
    diff.training_losses(model, cu(x))["loss"].mean().backward()
    opt.step()
    model.eval()
    after = score_candidates(diff, model, dcsr, ids, cand, mask=None, candidate_route="gathered")
    assert diff.last_candidate_route == "gathered"
    picked = score_candidates(diff, model, dcsr, ids, cand, mask=None, candidate_route="picked")
    ref = np.take_along_axis(_oracle64(monkeypatch, model, meta, x), cand.numpy(), 1)
    tol = 2e-5 * max(np.abs(ref).max(), 1.0)
    dev_g, dev_p = (np.abs(t.cpu().double().numpy() - ref).max() for t in (after, picked))
    moved = float((after - before).abs().max())
    print(f"after the step: gathered {dev_g:.3e}, picked {dev_p:.3e} from the oracle (tol {tol:.3e}); the step moved {moved:.3e}")
    assert dev_g <= tol and dev_p <= tol
    assert moved > 100 * tol  # the step really moved the result: stale operands cannot pass


def test_a_retrievers_lists_are_reranked_within_themselves():
    U, I, C, k = 12, 131, 30, 10
    rng = np.random.default_rng(5)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    uu, ii = train.nonzero()
    torch.manual_seed(3)
    retriever = gdmcf_amd.LightGCN({"user_id_idx": uu.astype(np.int64), "item_id_idx": ii.astype(np.int64)}, U, I, 2, 16,
                                   device=DEV).to(DEV)
    ids = torch.tensor([7, 0, 11, 3, 3])
    lists = retriever.recommend(ids, C, history=train)
    assert lists.shape == (len(ids), C) and lists.is_cuda
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=9)
    dcsr = DeviceCSR(train, DEV)
    val, idx = recommend(diff, model, dcsr, ids, k, candidates=lists, return_values=True)
    assert diff.last_candidate_route == "picked"  # 5 x 30 > 131
    val_g, idx_g = recommend(diff, model, dcsr, ids, k, candidates=lists, return_values=True, candidate_route="gathered")
    his = train.toarray() != 0
    for got_val, got in ((val, idx), (val_g, idx_g)):
        assert bool(torch.isfinite(got_val).all())
        for b, u in enumerate(ids.tolist()):
            items = got[b].tolist()
            assert set(items) <= set(lists[b].tolist()) and len(set(items)) == k
            assert not his[u, items].any()


def test_evaluate_with_candidates_gives_the_metrics_of_recommends_lists():
    U, I, bs, C, topN = 21, 131, 8, 30, [5, 10]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=2)
    cand = torch.from_numpy(np.stack([rng.permutation(I)[:C] for _ in range(U)]))
    got = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True, candidates=cand)
    lists = recommend(diff, model, DeviceCSR(train, DEV), np.arange(U), topN[-1], mask=DeviceCSR(train, DEV), batch_size=bs,
                      candidates=cand)
    truth = [test.indices[test.indptr[u]:test.indptr[u + 1]].tolist() for u in range(U)]
    want = evaluate_utils.computeTopNAccuracy(truth, lists.cpu().tolist(), topN)
    assert tuple(got) == tuple(want), (got, want)
    assert got != driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True)
    with pytest.raises(ValueError, match="recommend=True"):
        driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, candidates=cand)
