"""GPU (-m gpu): the fused LightGCN BPR step (csrc/bpr.hip, gdmcf_amd.lightgcn.BPRTrainer / bpr_loss_grad) against
oracle.lightgcn_bpr_step (CPU torch.sparse autograd) and against the autograd route around the same propagation kernels.
Tolerances are those of test_gpu_parity.py::test_lightgcn_bpr_step_gradients_match_oracle -- the same quantities against the
same oracle: |mf - ref| < 1e-6, |reg - ref| < 1e-4 ref, relerr(grad) < 1e-5.
The loss and scatter kernels alone, at every lane width, run length and stride: tests/test_gpu_bpr_kernels.py."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd.lightgcn import BPRTrainer, bpr_loss, bpr_loss_grad, bpr_reg_grad_, sample_bpr_batch, sample_bpr_items
from oracle import gdmcf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DECAY = 1e-4


def cu(a):
    return torch.as_tensor(a).to(DEV)


@functools.lru_cache(maxsize=None)
def main_graph():
    """The graph of test_lightgcn_bpr_step_gradients_match_oracle: (users, items, U, It, A~, R) and five batches of 128."""
    rng = np.random.default_rng(0)
    U, It, nnz = 400, 250, 5000
    users = np.concatenate([rng.integers(0, U, nnz), np.arange(U)])
    items = np.concatenate([np.minimum((rng.pareto(1.2, nnz) * It / 20).astype(np.int64), It - 1), rng.integers(0, It, U)])
    A = O.lightgcn_norm_adj(users, items, U, It)
    R = A[:U, U:].tocsr()
    batches = tuple(sample_bpr_batch(R.indptr, R.indices, U, It, 128, rng) for _ in range(5))
    return users, items, U, It, A, R, batches


@functools.lru_cache(maxsize=None)
def small_graph():
    """50 users x 7 items, 1-4 interactions each: with B = 128 every id repeats and items are pos and neg at once."""
    rng = np.random.default_rng(1)
    U, It = 50, 7
    rows = [rng.choice(It, size=int(rng.integers(1, 5)), replace=False) for _ in range(U)]
    users = np.concatenate([np.full(len(r), u) for u, r in enumerate(rows)])
    items = np.concatenate(rows)
    A = O.lightgcn_norm_adj(users, items, U, It)
    R = A[:U, U:].tocsr()
    return users, items, U, It, A, R, (sample_bpr_batch(R.indptr, R.indices, U, It, 128, rng),)


def model_of(graph, d, L=3, seed=0):
    users, items, U, It = graph[:4]
    torch.manual_seed(seed)
    return gdmcf_amd.LightGCN({"user_id_idx": users, "item_id_idx": items}, U, It, L, d, device=DEV).to(DEV)


def fused_loss_and_grad(m, bu, bp, bn):
    """(mf, reg, dE0, G) through bpr_loss_grad, the propagation of the cotangent and the regulariser rows."""
    E0 = m.E0.weight.detach()
    u, p, n = cu(bu), cu(bp), cu(bn)
    M = m._propagate(E0)[0]
    mf, reg, G = bpr_loss_grad(M, E0, u, p, n, m.n_users, DECAY)
    D = bpr_reg_grad_(m._propagate(G)[0], E0, u, p, n, m.n_users, DECAY)
    return mf, reg, D, G


def check_against_oracle(graph, m, bu, bp, bn):
    A, U = graph[4], graph[2]
    E0 = m.E0.weight.detach().cpu().numpy().copy()
    mf_ref, reg_ref, g_ref = O.lightgcn_bpr_step(A, E0, m.n_layers, U, bu, bp, bn, DECAY)
    mf, reg, D, G = fused_loss_and_grad(m, bu, bp, bn)
    assert mf.shape == () and reg.shape == () and mf.dtype == torch.float32
    err = (abs(float(mf) - mf_ref), abs(float(reg) - reg_ref) / reg_ref, H.relerr(D.cpu().numpy(), g_ref))
    print("bpr vs oracle: |mf - ref| %.3g  |reg - ref| / ref %.3g  relerr(grad) %.3g" % err)
    assert err[0] < 1e-6 and err[1] < 1e-4
    assert err[2] < 1e-5
    touched = np.zeros(U + graph[3], bool)
    touched[np.concatenate([bu, U + np.asarray(bp), U + np.asarray(bn)])] = True
    assert not G[cu(~touched)].any(), "rows of no triple must stay zero"
    return mf, reg, G


@pytest.mark.parametrize("d", [8, 64, 100, 10])
def test_loss_and_gradient_match_oracle(d):
    """d = 8: lane groups of 2; 64: the main path (16 lanes x float4); 100: the first-generation SpMM's width, a group with idle
    lanes; 10: the element-wise path."""
    g = main_graph()
    check_against_oracle(g, model_of(g, d), *g[6][0])


@pytest.mark.parametrize("case", ["all_repeat", "one_user_thrice", "single"])
def test_duplicates_are_summed_deterministically(case):
    g = small_graph()
    m = model_of(g, 64)
    if case == "all_repeat":
        bu, bp, bn = g[6][0]
        assert len(np.unique(bu)) < len(bu) and np.intersect1d(bp, bn).size > 0
    elif case == "one_user_thrice":  # pos[0] == neg[1]: item 2 is one run with a pos and a neg entry
        bu, bp, bn = np.array([3, 3, 3]), np.array([2, 4, 2]), np.array([5, 2, 6])
    else:
        bu, bp, bn = np.array([7]), np.array([1]), np.array([0])
    mf, reg, G = check_against_oracle(g, m, bu, bp, bn)
    mf2, reg2, _, G2 = fused_loss_and_grad(m, bu, bp, bn)
    assert torch.equal(mf, mf2) and torch.equal(reg, reg2) and torch.equal(G, G2)


def test_softplus_tails():
    """|x_j| > 20 with both signs: softplus is linear above torch's threshold and its derivative 1 there, exp(x) below -20;
    mf and coef against torch.nn.functional.softplus and its autograd on the CPU (float64, from the same table)."""
    U, It, d, B = 40, 30, 64, 128
    gen = torch.Generator().manual_seed(0)
    M = 0.3 * torch.randn(U + It, d, generator=gen)
    M[:5] *= 40.0  # five users whose scores are ~40 times the others'
    u = torch.randint(5, U, (B,), generator=gen)
    u[:10] = torch.arange(10) % 5
    p, n = torch.randint(0, It, (B,), generator=gen), torch.randint(0, It, (B,), generator=gen)
    x = ((M[u] * M[U + n]).sum(1) - (M[u] * M[U + p]).sum(1)).double().requires_grad_()
    assert (x > 20).any() and (x < -20).any()
    mf_ref = torch.nn.functional.softplus(x).mean()
    mf_ref.backward()
    Md = cu(M)
    mf, reg, G, coef = bpr_loss_grad(Md, Md, cu(u), cu(p), cu(n), U, DECAY, return_coef=True)
    for t in (mf, reg, G, coef):
        assert torch.isfinite(t).all()
    err = (abs(float(mf) - float(mf_ref)), H.relerr(coef.cpu().numpy(), x.grad.numpy()))
    print("softplus tails: mf %.6f  |mf - ref| %.3g  relerr(coef) %.3g" % (float(mf), *err))
    assert err[0] < 1e-6 and err[1] < 1e-5
    big = cu(x.detach() > 20)
    assert (coef[big] == 1.0 / B).all()
    # the negative tail, coef ~ exp(x) / B, is far below the largest coefficient, so relerr does not see it: element by element.
    # d coef / coef = dx, and x carries the float32 dot products' rounding: at most d = 64 roundings of half an ulp of a partial
    # sum below 128, 64 * 3.8e-6 = 2.5e-4 per product, 4.9e-4 for the two -- bound 1e-3
    assert float(x.detach().abs().max()) < 128
    low = x.detach() < -20
    rel = (coef.cpu().double()[low] / x.grad[low] - 1).abs().max()
    print("softplus tails: worst relative error of coef where x < -20: %.3g" % float(rel))
    assert (coef.cpu()[low] > 0).all() and float(rel) < 1e-3


def test_trainer_matches_the_autograd_route():
    g = main_graph()
    m1, m2 = model_of(g, 64), model_of(g, 64)
    assert torch.equal(m1.E0.weight, m2.E0.weight)
    tr = BPRTrainer(m1, g[5], batch_size=128, lr=0.005, decay=DECAY)
    opt = torch.optim.Adam(m2.parameters(), lr=0.005)
    for step, (bu, bp, bn) in enumerate(g[6]):
        mf1, reg1 = tr.step(bu, bp, bn)
        opt.zero_grad()
        out = m2(cu(bu), cu(bp), cu(bn))
        mf2, reg2 = bpr_loss(bu, *out)
        (mf2 + DECAY * reg2).backward()
        opt.step()
        err = (abs(float(mf1) - float(mf2)), H.relerr(m1.E0.weight.detach().cpu().numpy(), m2.E0.weight.detach().cpu().numpy()))
        print("step %d: |mf - mf_autograd| %.3g  relerr(E0) %.3g" % (step, *err))
        assert err[0] < 1e-6
        assert err[1] < 1e-5
    assert int(tr.flag) == 0 and tr.steps == 5
    with pytest.raises(IndexError):
        tr.step(np.array([0, g[2]]), np.array([0, 0]), np.array([1, 1]))
    with pytest.raises(IndexError):
        tr.step(np.array([0, 1]), np.array([0, -1]), np.array([1, 1]))


def test_two_trainers_with_one_seed_agree_bit_for_bit():
    g = main_graph()
    out = []
    for _ in range(2):
        m = model_of(g, 64)
        tr = BPRTrainer(m, g[5], batch_size=128, seed=11)
        for _ in range(5):
            tr.step()
        out.append(m.E0.weight.detach().clone())
    assert torch.equal(out[0], out[1])


def test_sharded_models_are_refused():
    m = model_of(small_graph(), 8)
    m._world = 2
    with pytest.raises(NotImplementedError):
        BPRTrainer(m, small_graph()[5])


def test_sampler_properties():
    """5 users x 12 items, degrees 1, 3, 6, 11 and 0; B = 6000 users drawn with replacement."""
    It, B = 12, 6000
    rows = [[4], [0, 5, 11], [1, 2, 3, 7, 8, 10], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11], []]
    uu = np.concatenate([np.full(len(r), u) for u, r in enumerate(rows)]).astype(np.int64)
    ii = np.concatenate([np.asarray(r, np.int64) for r in rows])
    R = sp.csr_matrix((np.ones(len(uu), np.float32), (uu, ii)), shape=(5, It))
    m = gdmcf_amd.LightGCN({"user_id_idx": uu, "item_id_idx": ii}, 5, It, 1, 8, device=DEV).to(DEV)
    tr = BPRTrainer(m, R, batch_size=B, seed=3)
    users, pos, neg = (t.cpu().numpy() for t in tr.sample())
    assert users.shape == pos.shape == neg.shape == (B,)
    assert (np.diff(users) >= 0).all() and set(users) == {0, 1, 2, 3}
    for u in range(4):
        sel = users == u
        n = int(sel.sum())
        inside, outside = rows[u], [i for i in range(It) if i not in rows[u]]
        assert np.isin(pos[sel], inside).all() and np.isin(neg[sel], outside).all()
        for drawn, cand in ((pos[sel], inside), (neg[sel], outside)):
            p = 1.0 / len(cand)
            sigma = np.sqrt(n * p * (1 - p))
            for c in cand:
                k = int((drawn == c).sum())
                assert k > 0 and abs(k - n * p) <= 5 * sigma, (u, c, k, n * p, sigma)
    assert int(tr.flag) == 0
    # same (seed, offset): the same items; the next offset: others
    ud = cu(users)
    a = sample_bpr_items(tr.indptr, tr.indices, ud, It, 3, 0)
    b = sample_bpr_items(tr.indptr, tr.indices, ud, It, 3, 0)
    c = sample_bpr_items(tr.indptr, tr.indices, ud, It, 3, 1)
    assert torch.equal(a[0], cu(pos)) and torch.equal(a[1], cu(neg))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # a user with nothing to draw: -1 and the flag
    pe, ne, fe = sample_bpr_items(tr.indptr, tr.indices, cu(np.array([1, 4])), It, 3, 0)
    assert int(pe[1]) == -1 and int(ne[1]) == -1 and int(fe) == 1 and int(pe[0]) in rows[1]


def test_sampler_draws_distinct_users_when_there_are_enough():
    rng = np.random.default_rng(2)
    U, It, B = 300, 40, 128
    rows = [rng.choice(It, size=int(rng.integers(1, 6)), replace=False) for _ in range(U)]
    rows[5], rows[9] = np.arange(It), np.zeros(0, np.int64)  # every item / none: not eligible
    uu = np.concatenate([np.full(len(r), u) for u, r in enumerate(rows)]).astype(np.int64)
    ii = np.concatenate(rows).astype(np.int64)
    R = sp.csr_matrix((np.ones(len(uu), np.float32), (uu, ii)), shape=(U, It))
    m = gdmcf_amd.LightGCN({"user_id_idx": uu, "item_id_idx": ii}, U, It, 1, 8, device=DEV).to(DEV)
    tr = BPRTrainer(m, R, batch_size=B, seed=0)
    seen = set()
    for _ in range(3):
        users, pos, neg = (t.cpu().numpy() for t in tr.sample())
        assert len(users) == B and (np.diff(users) > 0).all()
        assert 5 not in users and 9 not in users
        assert all(p in rows[u] and n not in rows[u] and 0 <= n < It for u, p, n in zip(users, pos, neg))
        seen.add(tuple(users))
    assert len(seen) == 3 and int(tr.flag) == 0


def test_resume_is_bit_exact():
    g = main_graph()
    m = model_of(g, 64)
    tr = BPRTrainer(m, g[5], batch_size=128, seed=5)
    for _ in range(3):
        tr.step()
    saved = dict(trainer=tr.state_dict(), model={k: v.clone() for k, v in m.state_dict().items()})
    saved["trainer"] = torch.load(_roundtrip(saved["trainer"]), weights_only=False)
    for _ in range(3):
        tr.step()
    m2 = model_of(g, 64, seed=99)
    m2.load_state_dict(saved["model"])
    tr2 = BPRTrainer(m2, g[5], batch_size=128, seed=0)
    tr2.load_state_dict(saved["trainer"])
    for _ in range(3):
        tr2.step()
    assert tr2.steps == 6 and torch.equal(m.E0.weight, m2.E0.weight)


def _roundtrip(obj):
    import io
    buf = io.BytesIO()
    torch.save(obj, buf)  # (also detaches the saved state from the live optimiser's tensors)
    buf.seek(0)
    return buf


def test_training_reduces_the_loss():
    g = main_graph()
    m = model_of(g, 64)
    tr = BPRTrainer(m, g[5], batch_size=128, lr=0.005, decay=DECAY)
    losses = torch.stack([tr.step()[0] for _ in range(30)]).cpu().numpy()
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
