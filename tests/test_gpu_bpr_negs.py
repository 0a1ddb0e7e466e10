"""GPU (-m gpu): several negatives per positive and dynamic ("hard") negatives on the device -- gdmcf_bpr_sample_pool_f32
(csrc/bpr.hip) through sample_bpr_negatives and BPRTrainer(n_negs=, neg_pool=), and BPRTrainer.train_epoch.  The draws are held
to the host Philox model of tests/bpr_negs_ref.py exactly; the step to oracle.lightgcn_bpr_step at the tolerances of
tests/test_gpu_bpr.py::check_against_oracle (the same quantities against the same oracle)."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from gdmcf_amd import bpr as bpr_module
from gdmcf_amd.lightgcn import BPRTrainer, sample_bpr_items, sample_bpr_negatives
from oracle import gdmcf_oracle as O
from tests import bpr_negs_ref as R
from tests import helpers as H
from tests import test_gpu_bpr as TB  # main_graph and model_of: the graph and models of the fused step's own tests

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY = TB.DECAY
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 13
OFFSETS = (5, (1 << 32) + 3)


def cu(a):
    return torch.as_tensor(a).to(DEV)


@functools.lru_cache(maxsize=None)
def edge_device():
    indptr, indices, U, It, users = R.edge_graph()
    return cu(indptr), cu(indices), cu(users)


@functools.lru_cache(maxsize=None)
def integer_table(d):
    """[37 + 53, d] float32 with entries in -2..2: every dot product is exact in float32 in any order, and scores tie"""
    return np.random.default_rng(d).integers(-2, 3, (37 + 53, d)).astype(np.float32)


def check_exact(d, n_negs, pool, table_on_device, M_host):
    indptr, indices, U, It, users = R.edge_graph()
    ip, ix, ud = edge_device()
    for offset in OFFSETS:
        pos, neg, flag = sample_bpr_negatives(ip, ix, ud, It, SEED, offset, n_negs=n_negs, pool=pool, M=table_on_device)
        rpos, rneg, rflag, cands = R.pool_triples(indptr, indices, users, U, It, SEED, offset, n_negs, pool, M_host)
        assert pos.shape == (33,) and neg.shape == (33, n_negs) and pos.dtype == neg.dtype == torch.int64
        assert np.array_equal(pos.cpu().numpy(), rpos), (d, n_negs, pool, offset)
        assert np.array_equal(neg.cpu().numpy(), rneg), (d, n_negs, pool, offset)
        assert int(flag) == rflag == 1
        if pool > 1:  # the case means something: pools with distinct candidates, and ties between distinct candidates, occur
            live = cands[:, :, 0] >= 0
            assert (cands[live].max(-1) != cands[live].min(-1)).any()


@pytest.mark.parametrize("n_negs,pool", [(1, 1), (3, 1), (1, 3), (1, 4), (3, 5)])
@pytest.mark.parametrize("d", [64, 8, 100, 10])
def test_draws_match_the_host_model_exactly(d, n_negs, pool):
    """d = 64: lane groups of 16; 8: of 2; 100: of 32 with idle lanes; 10: the element-wise path.  Candidate numbers 2, 3 and 14
    (the last word of block 0, the first of block 1, block 3) are met at (1, 3), (1, 4) and (3, 5)."""
    M = integer_table(d)
    check_exact(d, n_negs, pool, cu(M), M)


def test_draws_match_the_host_model_on_an_unaligned_table_view():
    """rows ldm = d + 1 apart, the first one float behind an aligned address: element-wise loads at d = 64"""
    d = 64
    M = integer_table(d)
    N = M.shape[0]
    store = torch.zeros(N * (d + 1) + 1, dtype=torch.float32, device=DEV)
    view = store[1:].view(N, d + 1)[:, :d]
    view.copy_(cu(M))
    assert view.stride() == (d + 1, 1) and view.data_ptr() % 16 == 4
    check_exact(d, 3, 5, view, M)


@pytest.mark.parametrize("n_negs,pool", [(1, 3), (3, 5), (2, 70)])
@pytest.mark.parametrize("d", [1, 3, 4, 12, 20, 200, 256, 260, 516])
def test_draws_match_the_host_model_at_every_lane_width(d, n_negs, pool):
    """The lane groups the test above leaves out -- d = 1, 3, 4: one lane; 12: four; 20: eight; 200, 256: a whole wave -- and two
    (260) and three (516) column passes, where the user row's first pass stays in registers and the rest is read again.  A pool
    of 70 is more than the widest lane group: two chunks of candidates.  |score| <= 4 d = 2064: exact."""
    M = integer_table(d)
    check_exact(d, n_negs, pool, cu(M), M)


def test_draws_match_the_host_model_on_an_unaligned_table_view_in_two_column_passes():
    """as the view above at d = 260: element-wise loads in both column passes"""
    d = 260
    M = integer_table(d)
    N = M.shape[0]
    store = torch.zeros(N * (d + 1) + 1, dtype=torch.float32, device=DEV)
    view = store[1:].view(N, d + 1)[:, :d]
    view.copy_(cu(M))
    assert view.stride() == (d + 1, 1) and view.data_ptr() % 16 == 4
    check_exact(d, 2, 70, view, M)


def test_ties_keep_the_earliest_drawn():
    indptr, indices, U, It, users = R.edge_graph()
    ip, ix, ud = edge_device()
    M = np.zeros((U + It, 64), np.float32)
    _, neg, _ = sample_bpr_negatives(ip, ix, ud, It, SEED, 0, n_negs=2, pool=5, M=cu(M))
    cands = R.pool_triples(indptr, indices, users, U, It, SEED, 0, 2, 5, M)[3]
    assert np.array_equal(neg.cpu().numpy(), cands[:, :, 0])
    M[:] = np.nan  # a NaN score never replaces anything
    _, neg, _ = sample_bpr_negatives(ip, ix, ud, It, SEED, 0, n_negs=2, pool=5, M=cu(M))
    assert np.array_equal(neg.cpu().numpy(), cands[:, :, 0])


@pytest.mark.parametrize("offset", OFFSETS)
def test_the_old_draw_is_the_special_case(offset):
    ip, ix, ud = edge_device()
    pos0, neg0, flag0 = sample_bpr_items(ip, ix, ud, 53, SEED, offset)
    pos, neg, flag = sample_bpr_negatives(ip, ix, ud, 53, SEED, offset)
    assert neg.shape == (33, 1)
    assert torch.equal(pos, pos0) and torch.equal(neg[:, 0], neg0) and int(flag) == int(flag0) == 1
    pos, neg, _ = sample_bpr_negatives(ip, ix, ud, 53, SEED, offset, n_negs=1, pool=1, M=cu(integer_table(64)))  # M is not read
    assert torch.equal(pos, pos0) and torch.equal(neg[:, 0], neg0)


def test_sampler_properties():
    """The 5 x 12 graph of test_gpu_bpr.py::test_sampler_properties, 2 000 drawn users.  The conditions are deterministic (fixed
    seed) and hold for the host model: tests/test_host_bpr_negs.py::test_statistical_conditions_hold_for_the_host_model."""
    indptr, indices, U, It, users = R.property_graph()
    ip, ix, ud = cu(indptr), cu(indices), cu(users)
    pos, neg, flag = sample_bpr_negatives(ip, ix, ud, It, 3, 0, n_negs=3, pool=1)
    assert int(flag) == 0 and neg.shape == (2000, 3)
    neg = neg.cpu().numpy()
    assert (neg >= 0).all() and (neg < It).all()
    assert all(p in R.PROPERTY_ROWS[u] for u, p in zip(users, pos.cpu().numpy()))
    R.check_uniform_negatives(users, neg)
    # scores that increase with the item id: the best of three is the largest of three
    M = R.increasing_score_table(U, It, 8)
    _, neg, flag = sample_bpr_negatives(ip, ix, ud, It, 3, 1, n_negs=3, pool=3, M=cu(M))
    cands = R.pool_triples(indptr, indices, users, U, It, 3, 1, 3, 3, M)[3]
    assert int(flag) == 0
    R.check_best_of_three(users, neg.cpu().numpy(), cands)


def test_real_valued_tables_choose_within_float32_rounding_of_the_best():
    """Normal-random table, d = 64, pool = 8.  The kernel's float32 scores carry at most d roundings each of half an ulp of a
    partial sum bounded by sum_i |a_i| |b_i|: |s32 - s| <= d 2^-24 sum_i |a_i| |b_i| in any summation order (products included:
    d + 1 roundings of relative size 2^-24 compound to less than that bound doubled).  Two scores are compared, so the chosen
    candidate's exact score lies no further below the pool's exact maximum than 2 d 2^-23 max_c sum_i |a_i| |b_ci|."""
    indptr, indices, U, It, users = R.edge_graph()
    ip, ix, ud = edge_device()
    d, pool, n_negs = 64, 8, 3
    M = np.random.default_rng(4).standard_normal((U + It, d)).astype(np.float32)
    _, neg, _ = sample_bpr_negatives(ip, ix, ud, It, SEED, 2, n_negs=n_negs, pool=pool, M=cu(M))
    _, neg1, _ = sample_bpr_items(ip, ix, ud, It, SEED, 2)
    neg, neg1 = neg.cpu().numpy(), neg1.cpu().numpy()
    cands = R.pool_triples(indptr, indices, users, U, It, SEED, 2, n_negs, pool, M)[3]
    T = M.astype(np.float64)
    worst, checked = 0.0, 0
    for j, u in enumerate(users.tolist()):
        if cands[j, 0, 0] < 0:
            assert (neg[j] == -1).all()
            continue
        for k in range(n_negs):
            assert neg[j, k] in cands[j, k]
            scores = T[U + cands[j, k]] @ T[u]
            bound = 2 * d * 2.0 ** -23 * (np.abs(T[U + cands[j, k]]) @ np.abs(T[u])).max()
            chosen = T[U + neg[j, k]] @ T[u]
            worst = max(worst, (scores.max() - chosen) / bound)
            assert chosen >= scores.max() - bound, (j, k)
            checked += 1
            if k == 0:  # candidate 0 of slot 0 is the pool = 1 draw: the pool can only do better
                assert cands[j, 0, 0] == neg1[j]
                assert chosen >= T[U + neg1[j]] @ T[u] - bound
    print("real-valued tables: %d slots, worst (max - chosen) / bound %.3g" % (checked, worst))
    assert checked > 60


@pytest.mark.parametrize("d", [64, 10])
@pytest.mark.parametrize("n_negs,neg_pool", [(3, 1), (2, 4)])
def test_step_matches_the_oracle(d, n_negs, neg_pool):
    g = TB.main_graph()
    A, U, It, Rcsr = g[4], g[2], g[3], g[5]
    kw = dict(batch_size=64, lr=0.005, decay=DECAY, seed=21, n_negs=n_negs, neg_pool=neg_pool)
    m0, m1, m2 = (TB.model_of(g, d) for _ in range(3))
    sampler = BPRTrainer(m0, Rcsr, **kw)
    users, pos, neg = sampler.sample()
    assert users.shape == pos.shape == neg.shape == (64 * n_negs,) and sampler.draws == 1
    bu, bp, bn = (t.cpu().numpy() for t in (users, pos, neg))
    assert (np.diff(bu) >= 0).all() and (bu.reshape(64, n_negs) == bu[::n_negs, None]).all()
    assert (bp.reshape(64, n_negs) == bp[::n_negs, None]).all()
    for u, p, n in zip(bu, bp, bn):
        row = Rcsr.indices[Rcsr.indptr[u]:Rcsr.indptr[u + 1]]
        assert p in row and n not in row and 0 <= n < It
    E0 = m1.E0.weight.detach().cpu().numpy().copy()
    mf_ref, reg_ref, g_ref = O.lightgcn_bpr_step(A, E0, m1.n_layers, U, bu, bp, bn, DECAY)
    fed = BPRTrainer(m1, Rcsr, **kw)
    mf, reg = fed.step(users, pos, neg)
    err = (abs(float(mf) - mf_ref), abs(float(reg) - reg_ref) / reg_ref, H.relerr(m1.E0.weight.grad.cpu().numpy(), g_ref))
    print("bpr step, n_negs %d pool %d d %d: |mf - ref| %.3g  |reg - ref| / ref %.3g  relerr(grad) %.3g" % (n_negs, neg_pool, d, *err))
    assert err[0] < 1e-6 and err[1] < 1e-4
    assert err[2] < 1e-5
    own = BPRTrainer(m2, Rcsr, **kw)
    mf2, reg2 = own.step()
    assert torch.equal(mf, mf2) and torch.equal(reg, reg2)
    assert torch.equal(m1.E0.weight.grad, m2.E0.weight.grad) and torch.equal(m1.E0.weight, m2.E0.weight)
    assert int(sampler.flag) == int(fed.flag) == int(own.flag) == 0 and own.draws == 1 and fed.draws == 0


def test_two_trainers_with_one_seed_agree_bit_for_bit():
    g = TB.main_graph()
    out = []
    for _ in range(2):
        m = TB.model_of(g, 64)
        tr = BPRTrainer(m, g[5], batch_size=128, seed=11, n_negs=2, neg_pool=3)
        for _ in range(5):
            tr.step()
        out.append(m.E0.weight.detach().clone())
    assert torch.equal(out[0], out[1])


def test_resume_is_bit_exact_with_the_same_knobs():
    g = TB.main_graph()
    kw = dict(batch_size=128, n_negs=2, neg_pool=3)
    m = TB.model_of(g, 64)
    tr = BPRTrainer(m, g[5], seed=5, **kw)
    for _ in range(3):
        tr.step()
    saved = dict(trainer=tr.state_dict(), model={k: v.clone() for k, v in m.state_dict().items()})
    assert set(saved["trainer"]) == {"optimizer", "steps", "draws", "seed", "generator"}
    saved["trainer"] = torch.load(TB._roundtrip(saved["trainer"]), weights_only=False)
    for _ in range(3):
        tr.step()
    m2 = TB.model_of(g, 64, seed=99)
    m2.load_state_dict(saved["model"])
    tr2 = BPRTrainer(m2, g[5], seed=0, **kw)
    tr2.load_state_dict(saved["trainer"])
    for _ in range(3):
        tr2.step()
    assert tr2.steps == 6 and tr2.draws == 6 and torch.equal(m.E0.weight, m2.E0.weight)


def test_the_default_trainer_is_untouched(monkeypatch):
    calls = dict(old=0, new=0)
    old, new = bpr_module._bpr_sample, bpr_module._bpr_sample_pool
    lib_new = bpr_module._lib.load().gdmcf_bpr_sample_pool_f32

    def count(name, f):
        def wrapped(*a, **k):
            calls[name] += 1
            return f(*a, **k)
        return wrapped

    monkeypatch.setattr(bpr_module, "_bpr_sample", count("old", old))
    monkeypatch.setattr(bpr_module, "_bpr_sample_pool", count("new", new))
    monkeypatch.setattr(bpr_module._lib.load(), "gdmcf_bpr_sample_pool_f32", count("new", lib_new))
    g = TB.main_graph()
    out = []
    for kw in (dict(), dict(n_negs=1, neg_pool=1)):
        m = TB.model_of(g, 64)
        tr = BPRTrainer(m, g[5], batch_size=128, seed=11, **kw)
        shapes = [t.shape for t in tr.sample()]
        assert shapes == [(128,)] * 3
        for _ in range(5):
            tr.step()
        out.append(m.E0.weight.detach().clone())
    assert torch.equal(out[0], out[1])
    assert calls == dict(old=12, new=0)
    with pytest.raises(ValueError):
        BPRTrainer(TB.model_of(g, 8), g[5], n_negs=0)
    with pytest.raises(ValueError):
        BPRTrainer(TB.model_of(g, 8), g[5], neg_pool=0)


@pytest.mark.parametrize("kw", [dict(), dict(n_negs=2, neg_pool=3)], ids=["default", "negs2_pool3"])
def test_train_epoch_is_ten_steps_and_does_not_synchronise(kw):
    """Synchronisations are recorded as tests/test_gpu_rank.py records them (sync debug mode "warn")."""
    g = TB.main_graph()
    m1, m2 = TB.model_of(g, 64), TB.model_of(g, 64)
    t1 = BPRTrainer(m1, g[5], batch_size=128, seed=8, **kw)
    t2 = BPRTrainer(m2, g[5], batch_size=128, seed=8, **kw)
    pairs = [t2.step() for _ in range(10)]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as seen:  # (every synchronising torch call leaves one warning here)
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            mf, reg = t1.train_epoch(10)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    # FusedAdamW (unchanged here) uploads its pointer table from pageable memory whenever the fresh gradient table lands at an
    # address it has not seen: a handful of times per run, whichever way the steps are called.  Nothing else may synchronise:
    # not the sampler, the propagation, the loss, the sort, the scatter, nor the epoch's accumulation of the losses.
    syncs = [w for w in seen if "called a synchronizing" in str(w.message)]
    foreign = [(w.filename, w.lineno) for w in syncs if not w.filename.endswith(os.path.join("gdmcf_amd", "optim.py"))]
    print("train_epoch(10): %d synchronising calls, %d outside the optimiser's table upload" % (len(syncs), len(foreign)))
    assert not foreign, foreign
    assert mf.shape == reg.shape == () and mf.dtype == reg.dtype == torch.float32 and mf.is_cuda
    assert t1.steps == t1.draws == 10 and torch.equal(m1.E0.weight, m2.E0.weight)
    # a float32 mean of ten float32 values: nine additions, each rounding at most half an ulp of a partial sum below sum |v|,
    # and the division's one rounding: |mean32 - mean| <= 2^-24 (0.9 sum |v| + |mean|)
    for got, vals in ((mf, [p[0] for p in pairs]), (reg, [p[1] for p in pairs])):
        v = np.array([float(x) for x in vals], dtype=np.float64)
        assert abs(float(got) - v.mean()) <= 2.0 ** -24 * (0.9 * np.abs(v).sum() + abs(v.mean())), (float(got), v.mean())


def test_example_trains_and_evaluates():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lightgcn_synthetic.py"), "--users", "300", "--items",
                        "120", "--epochs", "2", "--n-negs", "2", "--neg-pool", "4"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2, r.stdout
    for ln in lines:
        fields = dict(f.split("=") for f in ln.split()[2:])
        assert {"mf", "reg", "recall@20", "ndcg@20"} <= set(fields)
        assert all(np.isfinite(float(v)) for v in fields.values()), ln
