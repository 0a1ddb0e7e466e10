"""CPU (-m "not gpu"): the host reference of the BPR kernels (tests/bpr_ref.py) is right, and the comparisons that
tests/test_gpu_bpr_kernels.py makes with it mean something -- the float64 formulas equal torch autograd of gdmcf_amd.bpr.bpr_loss
and its index_put_ scatters, every batch builder builds the runs its name promises at every lane-group size, the dyadic tables are
exact in float32 in any order, and check_loss / check_mode0 / check_mode1 pass a plain float32 evaluation while they reject a
dropped or duplicated entry, a run cut at LG entries, a neighbour's row and a dropped column chunk."""
import numpy as np
import pytest
import torch

from gdmcf_amd.bpr import bpr_loss
from tests import bpr_ref as R

DECAY = 2.0 ** -4
HOST_TOL = 4 * R.U  # a correctly rounded sigmoid, softplus and division: well inside


def tables(b, d, kind="dyadic"):
    make = dict(dyadic=R.dyadic_table, tails=R.tails_table, real=R.real_table)[kind]
    return make(b.N, d, 1), R.dyadic_table(b.N, d, 2) if kind != "real" else R.real_table(b.N, d, 2)


def autograd(M, E0, b):
    """(mf, reg, coef, G, Rg) of torch float64 autograd around bpr_loss: coef = d mf / d x, G = the six index_put_ scatters of
    the embeddings' cotangents under mf, Rg = those of reg"""
    T, E = torch.tensor(np.asarray(M, np.float64)), torch.tensor(np.asarray(E0, np.float64))
    u, p, n = (torch.tensor(a) for a in (b.users, b.n_users + b.pos, b.n_users + b.neg))
    leaves = [t.clone().requires_grad_(True) for t in (T[u], T[p], T[n], E[u], E[p], E[n])]
    mf, reg = bpr_loss(b.users, *leaves)
    G, Rg = torch.zeros_like(T), torch.zeros_like(E)
    for table, loss, ls in ((G, mf, leaves[:3]), (Rg, reg, leaves[3:])):
        for idx, cot in zip((u, p, n), torch.autograd.grad(loss, ls)):
            table.index_put_((idx,), cot, accumulate=True)
    # d mf / d x: the same function on one-column "embeddings", x = neg score - pos score
    sp, sn = (T[u] * T[p]).sum(1), ((T[u] * T[n]).sum(1)).requires_grad_(True)
    one = torch.ones(b.B, 1, dtype=torch.float64)
    mf1, _ = bpr_loss(b.users, one, sp[:, None], sn[:, None], one, one, one)
    coef, = torch.autograd.grad(mf1, sn)
    assert abs(float(mf1.detach()) - float(mf.detach())) <= 1e-12 * abs(float(mf.detach()))
    return float(mf.detach()), float(reg.detach()), coef.numpy(), G.numpy(), Rg.numpy()


@pytest.mark.parametrize("kind,d", [("dyadic", 64), ("tails", 64), ("tails", 20), ("real", 100)])
def test_loss_reference_is_autograd_of_bpr_loss(kind, d):
    b = R.spread(128)
    if kind == "tails":
        b = R.Batch("spread", b.users % 8, b.pos, b.neg, b.n_users, b.n_items)
    M, E0 = tables(b, d, kind)
    ref = R.loss_ref(M, E0, b)
    mf, reg, coef, _, _ = autograd(M, E0, b)
    assert abs(ref["mf"] - mf) <= 1e-13 * abs(mf) and abs(ref["reg"] - reg) <= 1e-13 * reg
    assert np.allclose(ref["coef"], coef, rtol=1e-12, atol=0) and ref["flag"] == 0 and ref["ok"].all()
    if kind == "tails":
        assert (ref["x"] > 20).any() and (ref["x"] < -20).any()


@pytest.mark.parametrize("name", ["spread", "hub_item", "bad_ids"])
def test_scatter_references_are_the_index_put_scatters_of_autograd(name):
    d = 20
    b = dict(spread=R.spread(65), hub_item=R.hub_item(9), bad_ids=R.bad_ids(65))[name]
    c = b.clean()
    assert (name == "bad_ids") == (c.B < b.B) and c.ok().all()
    M, E0 = tables(b, d, "real")
    ref = R.loss_ref(M, E0, b)
    mf, reg, coef, G, Rg = autograd(M, E0, c)
    part = c.B / b.B  # the bad triples dropped: the same sums, divided by the whole batch's B
    assert abs(ref["mf"] - mf * part) <= 1e-13 * mf and abs(ref["reg"] - reg * part) <= 1e-13 * reg
    assert np.allclose(ref["coef"][b.ok()], coef * part, rtol=1e-12, atol=0) and (ref["coef"][~b.ok()] == 0).all()
    out, written, mag, count = R.mode0_ref(b, ref["coef"], M, np.zeros_like(M))
    assert np.allclose(out, G * part, rtol=0, atol=1e-13) and (np.abs(out) <= mag + 1e-15).all()
    assert np.array_equal(written, count > 0) and np.array_equal(count, b.multiplicity())
    sentinel = np.full_like(M, 7.5)
    assert (R.mode0_ref(b, ref["coef"], M, sentinel)[0][~written] == 7.5).all()
    out1, zero = R.mode1_ref(b, E0, out, DECAY / b.B, np.ones_like(M))
    assert np.array_equal(zero == 0, np.repeat(written[:, None], d, 1))
    if name != "bad_ids":  # (an entry of a bad triple whose own id is valid still counts in the regulariser's multiplicity)
        assert np.allclose(out1, (G + DECAY * Rg) * part, rtol=0, atol=1e-13)
        # propagation-free: one table as M and as E0, the dense gradient of mf + decay reg
        T = torch.tensor(np.asarray(M, np.float64), requires_grad=True)
        u, p, n = (torch.tensor(a) for a in (b.users, b.n_users + b.pos, b.n_users + b.neg))
        mf_t, reg_t = bpr_loss(b.users, T[u], T[p], T[n], T[u], T[p], T[n])
        (mf_t + DECAY * reg_t).backward()
        same = R.loss_ref(M, M, b)
        dense = R.mode1_ref(b, M, R.mode0_ref(b, same["coef"], M, np.zeros_like(M))[0], DECAY / b.B)[0]
        assert np.allclose(dense, T.grad.numpy(), rtol=0, atol=1e-13)
    else:
        counts = np.bincount(np.concatenate([c.users, c.n_users + c.pos, c.n_users + c.neg]), minlength=b.N)
        extra = count - counts
        assert extra.sum() > 0 and np.allclose(out1 - (DECAY / b.B) * extra[:, None] * E0, (G + DECAY * Rg) * part, rtol=0, atol=1e-13)


@pytest.mark.parametrize("LG", R.LGS)
def test_builders_build_what_their_names_say(LG):
    G = 256 // LG
    assert all(R.lane_group(d) == LG for d in R.WIDTHS[LG]) and set(R.SCATTER_WIDTHS) <= set(R.ALL_WIDTHS)
    assert sum(R.lane_group(d) == LG for d in R.SCATTER_WIDTHS) == (4 if LG == 64 else 1)
    batches = {b.name: b for b in R.scatter_batches(LG)}
    assert len(batches) == 9
    lengths = {}
    for b in batches.values():
        runs, od, nd = b.runs(), b.order(), b.nodes()
        assert sorted(od.tolist()) == list(range(3 * b.B)) and b.B < 600
        nodes = [r[0] for r in runs]
        assert len(set(nodes)) == len(nodes) and nodes == sorted(nodes)  # no run is split by an out-of-range entry
        assert all((np.diff(od[s:s + n]) > 0).all() for _, s, n in runs)  # entries of a node in ascending e
        assert np.array_equal(np.bincount(nodes, weights=[r[2] for r in runs], minlength=b.N), b.multiplicity())
        lengths[b.name] = {node: (s, n) for node, s, n in runs}
    assert any((3 * b.B) % G for b in batches.values()) and (3 * batches["spread"].B) % G and (3 * batches["bad_ids"].B) % G
    assert np.mean([n <= 2 for _, n in lengths["spread"].values()]) > 0.6 and len(lengths["spread"]) > batches["spread"].B
    b = batches["hub_user"]
    assert lengths["hub_user"][5] == (0, b.B) and b.B > 2 * LG
    b = batches["hub_item"]
    assert lengths["hub_item"][b.n_users + 3][1] == 2 * b.B and b.B == LG + 1
    got = [lengths["multiples"][u][1] for u in range(len(R.multiple_lengths(LG)))]
    assert got == R.multiple_lengths(LG) and {1, LG, LG + 1, 2 * LG, 2 * LG + 1} <= set(got) and (LG == 1 or LG - 1 in got)
    for k in (1, 2):
        b = batches["last_run_full%d" % k]
        s, n = lengths[b.name][b.N - 1]
        assert n == k * LG and s + n == 3 * b.B
    b = batches["straddle"]
    s, n = lengths["straddle"][10]
    assert s == G - 1 and n >= LG + 2 and s + n > G
    b = batches["neighbours"]
    (s0, n0), (s1, n1) = lengths["neighbours"][b.n_users - 1], lengths["neighbours"][b.n_users]
    assert n0 == LG and s0 + n0 == s1 and n1 == 3
    # the multiplicities the mode-1 test needs
    seen = set().union(*[set(n for _, n in v.values()) for v in lengths.values()])
    assert {1, LG, LG + 1, 2 * LG, 2 * batches["hub_item"].B} <= seen


@pytest.mark.parametrize("B", [1, 5, 9, 18, 128, 257])
def test_bad_ids_has_what_the_kernel_tests_need(B):
    b = R.bad_ids(B)
    ok, nd, od = b.ok(), b.nodes(), b.order()
    assert 0 < (~ok).sum() <= max(1, min(9, B // 2 if B < 18 else 9)) and (B == 1 or ok.any())
    if B < 18:
        return
    U_, I_ = R.WIDE
    assert {-1, -3, U_, U_ + 2} <= set(b.users.tolist()) and {-3, I_, 2 ** 40} <= set(b.pos.tolist())
    assert {-3, I_, 2 ** 40} <= set(b.neg.tolist()) and ((b.users == U_) & (b.neg == 2 ** 40)).any() and (~ok).sum() == 9
    # entries whose key collides with a valid node's: directly behind user n_users - 3's run, directly before item 0's
    sorted_nodes = nd[od]
    runs = {node: (s, n) for node, s, n in b.runs()}
    s, n = runs[U_ - 3]
    assert n >= 2 and (sorted_nodes[s + n:s + n + 2] == -1).all() and set(od[s + n:s + n + 2]) == {B + 4, 2 * B + 2}
    s, n = runs[U_]
    assert n >= 2 and sorted_nodes[s - 1] == -1 and od[s - 1] == 3


def test_loss_batches():
    for LG in R.LGS:
        G = 256 // LG
        bs = R.loss_batches(LG)
        assert sorted({b.B for b in bs}) == sorted({1, G + 1, 128}) and [b.name for b in bs] == ["spread", "hub_item", "bad_ids"] * 3
        assert all(b.ok().all() == (b.name != "bad_ids") for b in bs)


@pytest.mark.parametrize("d", R.ALL_WIDTHS)
def test_dyadic_tables_are_exact_in_any_order(d):
    """x and rg of every loss batch: float32 sums in a scrambled column order equal the float64 values; |x| < 10 on the dyadic
    table; with more than one column pass, zeroing the columns from 256 on changes x for at least half the triples"""
    perm = np.random.default_rng(d).permutation(d)
    tails = [0, 0]
    for b in R.loss_batches(R.lane_group(d))[3:]:
        for kind in ("dyadic", "tails"):
            M, E0 = tables(b, d, kind)
            ref = R.loss_ref(M, E0, b)
            ok, u, p, n = R._rows(b)
            Ms, Es = M[:, perm], E0[:, perm]
            x32 = np.where(ok, R.dot32(Ms[u], Ms[n]) - R.dot32(Ms[u], Ms[p]), 0)
            rg32 = np.where(ok, R.dot32(Es[u], Es[u]) + R.dot32(Es[p], Es[p]) + R.dot32(Es[n], Es[n]), 0)
            assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64), ref["x"]), kind
            assert np.array_equal(rg32.astype(np.float64), ref["rg"]) and float(np.float32(ref["rg"].sum())) == ref["rg"].sum()
            if kind == "dyadic":
                assert np.abs(ref["x"]).max() < 10
                if d > 256 and b.name == "spread" and b.B == 128:
                    cut = M.copy()
                    cut[:, 256:] = 0
                    assert (R.loss_ref(cut, E0, b)["x"] != ref["x"]).sum() >= b.B / 2
                if b.name == "hub_item":
                    assert (ref["x"] == 0).all() and (ref["coef"] == 0.5 / b.B).all()
            else:
                tails[0] += int((ref["x"] > 20).sum())
                tails[1] += int((ref["x"] < -20).sum())
    if d >= 12:  # (below that a product of 16 and a difference of at most 1 per column rarely gets there)
        assert min(tails) > 0, tails


@pytest.mark.parametrize("d", [3, 20, 64, 129, 260])
def test_loss_comparison_passes_float32_and_rejects_a_dropped_chunk(d):
    for kind in ("dyadic", "tails", "real"):
        for b in (R.spread(65), R.bad_ids(65)):
            M, E0 = tables(b, d, kind)
            ref = R.loss_ref(M, E0, b)
            exact = kind != "real"
            got = R.loss32(M, E0, b, scramble=np.random.default_rng(d).permutation(d) if exact else None)
            R.check_loss(*got, ref, d, HOST_TOL, exact_x=exact, exact_reg=exact)
            if d > 3:
                with pytest.raises(AssertionError):
                    R.check_loss(*R.loss32(M, E0, b, fault="chunk"), ref, d, HOST_TOL, exact_x=exact, exact_reg=exact)
            # ... and a flagged triple that contributes, a wrong /B, an mf that misses a term
            coef, ws, mf, reg = got
            for wrong in ((coef * np.float32(b.B / (b.B + 1)), ws, mf, reg), (coef, ws, np.float32(mf - ws[:b.B].max() / b.B), reg),
                          (coef, ws, mf, np.float32(reg * (1 + 2 ** -22)))):
                if kind == "real" and wrong[3] is not reg:
                    continue
                with pytest.raises(AssertionError):
                    R.check_loss(*wrong, ref, d, HOST_TOL, exact_x=exact, exact_reg=exact)
            if b.name == "bad_ids":
                bad = np.flatnonzero(~b.ok())[0]
                ws2 = ws.copy()
                ws2[b.B + bad] = 1
                with pytest.raises(AssertionError):
                    R.check_loss(coef, ws2, mf, reg, ref, d, HOST_TOL, exact_x=exact, exact_reg=exact)


@pytest.mark.parametrize("d", [5, 16, 33, 260])
def test_scatter_comparisons_pass_float32_and_reject_every_fault(d):
    LG = R.lane_group(d)
    for b in R.scatter_batches(LG):
        src, isrc = R.dyadic_table(b.N, d, 3), R.int_table(b.N, d, 4)
        coef = np.where(b.ok(), R.dyadic_coef(b.B, 5), 0).astype(np.float32)
        out0, iout0 = np.full((b.N, d), -77.25, np.float32), R.int_table(b.N, d, 6, -5, 5)
        zero0 = R.int_table(b.N, d, 8, 1, 4)
        real, rcoef = R.real_table(b.N, d, 3), R.loss32(R.real_table(b.N, d, 3), R.real_table(b.N, d, 3), b)[0]
        R.check_mode0(R.scatter32(b, 0, coef, src, out0, LG)[0], b, coef, src, out0)
        R.check_mode0(R.scatter32(b, 0, rcoef, real, out0, LG)[0], b, rcoef, real, out0, exact=False)
        R.check_mode1(*R.scatter32(b, 1, None, isrc, iout0, LG, 2.0 ** -7, zero0), b, isrc, iout0, 2.0 ** -7, zero0)
        R.check_mode1(*R.scatter32(b, 1, None, isrc, iout0, LG, 2.0 ** -7), b, isrc, iout0, 2.0 ** -7)
        if b.name not in ("multiples", "straddle"):
            continue
        for fault in R.FAULTS:
            with pytest.raises(AssertionError):
                R.check_mode0(R.scatter32(b, 0, coef, src, out0, LG, fault=fault)[0], b, coef, src, out0)
            with pytest.raises(AssertionError):
                R.check_mode0(R.scatter32(b, 0, rcoef, real, out0, LG, fault=fault)[0], b, rcoef, real, out0, exact=False)
            with pytest.raises(AssertionError):
                R.check_mode1(*R.scatter32(b, 1, None, isrc, iout0, LG, 2.0 ** -7, zero0, fault=fault), b, isrc, iout0, 2.0 ** -7,
                              zero0)
    # a row of no entry that is written, and a zero_rows row cleared outside the batch
    b = R.multiples(LG)
    src, out0 = R.dyadic_table(b.N, d, 3), np.full((b.N, d), -77.25, np.float32)
    coef = R.dyadic_coef(b.B, 5)
    got = R.scatter32(b, 0, coef, src, out0, LG)[0]
    free = int(np.flatnonzero(b.multiplicity() == 0)[0])
    got[free, 0] = 0
    with pytest.raises(AssertionError):
        R.check_mode0(got, b, coef, src, out0)
