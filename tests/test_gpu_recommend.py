"""GPU: gdmcf_amd.recommend.  gdmcf_topk_masked_rows_f32 against gdmcf_topk_masked_f32 on the sub-CSR, bit for bit,
on both selection paths; its `scale`; recommend against the CPU oracle in float64 for the four backbones under a criterion that
covers every row; the routes and what the "latent-csr" route no longer launches; chunking and id order; driver.evaluate(recommend=
True); freshness after an optimiser step."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import _lib, driver, evaluate_utils
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import recommend
from oracle import gdmcf_oracle as O
from tests import helpers as H
from tests.test_gpu_latent import _discrete, _fresh_dnn, _oracle64, _oracle_discrete64, _rows, cu, dnn_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------------
# the kernel against the existing kernel
# ---------------------------------------------------------------------------------------------------------------------
N_USERS = 9
EMPTY, SHORT, MESSY = 2, 5, 7  # the special rows of the full CSR


def _raw_csr(I, k, seed, special=True):
    """(indptr, indices) of a CSR with N_USERS rows, built by hand so that nothing is canonicalised: row EMPTY has no entry, row
    SHORT leaves k - 1 items unmasked, row MESSY lists its items unsorted and some of them twice."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(N_USERS):
        r = np.flatnonzero(rng.random(I) < 0.15)
        if special and u == EMPTY:
            r = r[:0]
        elif special and u == SHORT:
            r = rng.permutation(I)[: I - (k - 1)]
        elif special and u == MESSY:
            r = rng.permutation(np.concatenate([r, r[: max(1, len(r) // 2)], rng.integers(0, I, 3)]))
        rows.append(r.astype(np.int32))
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32), rows


def _rows_call(pred, I, k, csr1, csr2, rows, scale=None):
    B = pred.shape[0]
    idx = torch.full((B, k), -7, dtype=torch.int64, device=DEV)
    val = torch.full((B, k), float("nan"), dtype=torch.float32, device=DEV)
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)
    ip1, ix1 = (t(csr1[0], torch.int64), t(csr1[1], torch.int32)) if csr1 is not None else (None, None)
    ip2, ix2 = (t(csr2[0], torch.int64), t(csr2[1], torch.int32)) if csr2 is not None else (None, None)
    rows_t = t(rows, torch.int64)
    _lib.check(_lib.load().gdmcf_topk_masked_rows_f32(
        pred.data_ptr(), pred.stride(0), B, I, _lib.ptr(ip1), _lib.ptr(ix1), _lib.ptr(ip2), _lib.ptr(ix2), _lib.ptr(rows_t),
        _lib.ptr(scale), k, idx.data_ptr(), val.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return val, idx


def _pred_in_wide_buffer(B, I, seed, ties):
    """[B, I] scores inside a NaN-filled buffer with an odd row stride; `ties`: small integers, so that many scores are equal."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((B, I + 13), float("nan"))
    buf[:, :I] = torch.randint(-3, 4, (B, I), generator=g).float() if ties else torch.randn(B, I, generator=g)
    return cu(buf)[:, :I]


KERNEL_CASES = [(I, k, B) for I in (5, 131, 1030, 4099, 40961) for k in sorted({1, 20, 256, 257, min(I, 1024)}) if k <= I
                for B in (1, 7)]


@pytest.mark.parametrize("I,k,B", KERNEL_CASES)
def test_rows_kernel_equals_masked_topk_on_the_sub_csr(I, k, B):
    """I = 40 961 is one past the fast path's width and k = 257 one past its k: both selection paths, and the fast path's hand-over
    of degenerate rows (SHORT; all-equal rows under `ties`), serve the entry."""
    ip1, ix1, rows1 = _raw_csr(I, k, 1)
    ip2, ix2, rows2 = _raw_csr(I, k, 2, special=False)
    picks = [[8, EMPTY, SHORT, EMPTY, 0, MESSY, 3]] if B == 7 else [[EMPTY], [SHORT], [MESSY]]  # unsorted, with a repeat
    for rows in picks:
        rows = np.asarray(rows, dtype=np.int64)
        sub = lambda rr: (np.concatenate([[0], np.cumsum([len(rr[u]) for u in rows])]).astype(np.int64),
                          np.concatenate([rr[u] for u in rows]).astype(np.int32))
        both = (sp.csr_matrix((np.ones(len(ix1)), ix1, ip1), shape=(N_USERS, I))
                + sp.csr_matrix((np.ones(len(ix2)), ix2, ip2), shape=(N_USERS, I)))[rows]
        for ties in (True, False):
            pred = _pred_in_wide_buffer(B, I, 10 * I + k + int(ties), ties)
            assert pred.stride(0) > I
            for csr_a, csr_b, want_csr in (((ip1, ix1), None, sub(rows1)), ((ip1, ix1), (ip2, ix2), (both.indptr, both.indices)),
                                           (None, None, None)):
                # (a sub-CSR without any entry gets one index that no indptr range covers: an empty tensor has no pointer)
                want = evaluate_utils.masked_topk(pred, k, torch.from_numpy(want_csr[0]),
                                                  torch.from_numpy(np.append(want_csr[1], 0).astype(np.int32)), return_values=True) \
                    if want_csr is not None else evaluate_utils.masked_topk(pred, k, return_values=True)
                val, idx = _rows_call(pred, I, k, csr_a, csr_b, rows)
                assert torch.equal(idx, want[1]), (rows, ties, csr_b is not None)
                assert torch.equal(val, want[0])  # (no NaN may appear: the padding is never read; -inf rows compare equal)
            if SHORT in rows:
                b = list(rows).index(SHORT)
                assert bool(torch.isinf(_rows_call(pred, I, k, (ip1, ix1), None, rows)[0][b, -1]))  # a masked item came back
    # rows == NULL: pred row b takes CSR row b
    pred = _pred_in_wide_buffer(B, I, 5, True)
    want = evaluate_utils.masked_topk(pred, k, torch.from_numpy(ip1[: B + 1]), torch.from_numpy(ix1), return_values=True)
    val, idx = _rows_call(pred, I, k, (ip1, ix1), None, None)
    assert torch.equal(idx, want[1]) and torch.equal(val, want[0])


@pytest.mark.parametrize("I,k", [(131, 20), (4099, 257), (40961, 20)])
def test_rows_kernel_scale_multiplies_the_returned_values_only(I, k):
    ip1, ix1, _ = _raw_csr(I, k, 3)
    rows = np.asarray([8, EMPTY, SHORT, EMPTY, 0, MESSY, 3], dtype=np.int64)
    pred = _pred_in_wide_buffer(7, I, 77, False)
    scale = cu(torch.rand(7, generator=torch.Generator().manual_seed(1)) + 0.5)
    val, idx = _rows_call(pred, I, k, (ip1, ix1), None, rows)
    val_s, idx_s = _rows_call(pred, I, k, (ip1, ix1), None, rows, scale=scale)
    assert torch.equal(idx_s, idx)
    assert torch.equal(val_s, val * scale[:, None])  # one float32 multiplication each; -inf stays -inf


# ---------------------------------------------------------------------------------------------------------------------
# recommend against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def _check_lists(val, idx, ref, masked, k, what):
    """The criterion of every row.  ref: the oracle's x_0 [n, I] (float64); masked: bool [n, I]; tol: the latent route's bound."""
    val, idx = val.cpu().double().numpy(), idx.cpu().numpy()
    tol = 2e-5 * max(np.abs(ref).max(), 1.0)
    ref = np.where(masked, -np.inf, ref)
    assert idx.shape == (ref.shape[0], k) and val.shape == idx.shape
    worst = 0.0
    for b in range(ref.shape[0]):
        items = idx[b]
        assert len(set(items.tolist())) == k, (what, b, "duplicates")
        assert items.min() >= 0 and items.max() < ref.shape[1]
        if (~masked[b]).sum() >= k:
            assert not masked[b, items].any(), (what, b, "a masked item although k items are unmasked")
        kth = np.sort(ref[b])[-k]
        assert ref[b, items].min() >= kth - 2 * tol, (what, b, ref[b, items].min(), kth)
        fin = np.isfinite(ref[b, items])
        assert np.array_equal(val[b][~fin], ref[b, items][~fin]), (what, b, "masked items carry -inf")
        if fin.any():
            worst = max(worst, np.abs(val[b][fin] - ref[b, items][fin]).max())
        assert np.abs(val[b][fin] - ref[b, items][fin]).max(initial=0.0) <= tol, (what, b)
        for j in range(k - 1):
            assert val[b, j] > val[b, j + 1] or (val[b, j] == val[b, j + 1] and items[j] < items[j + 1]), (what, b, j)
    print(f"{what}: worst value deviation {worst:.3e}, tol {tol:.3e}")


def _draws(B, I):
    g = torch.Generator().manual_seed(17)
    return torch.randn(B, I, generator=g), (torch.rand(B, I, generator=g) < 0.1).long()


def _user_csr(x, index, U):
    """DeviceCSR with U rows whose row index[b] is x[b]: recommend's user id is both the row and the model's `index`."""
    full = np.zeros((U, x.shape[1]), dtype=np.float64)
    full[np.asarray(index)] = np.asarray(x, dtype=np.float64)
    return DeviceCSR(sp.csr_matrix(full), DEV)


def _case(name, monkeypatch):
    """(model, diffusion, x [B, I] float32 on the host, user ids, DeviceCSR, ref_of(steps, noise0, sampled0))"""
    if name in ("dnn_tiny", "dnn_ragged", "dnn_deep"):
        if name == "dnn_deep":
            model, diff, meta = _fresh_dnn(131, [24, 40], [40, 24], 5, seed=3)
            x = _rows(10, 131, 1)
        else:
            fx = H.load("sample_tiny_x0" if name == "dnn_tiny" else "sample_ragged_x0")
            meta = H.sample_meta(fx)
            model, diff = dnn_pair(meta, fx)
            meta = dict(meta, dims_in=meta["dims"], dims_out=meta["dims"][::-1])
            x = torch.from_numpy(fx["x_start"].astype(np.float32))
        ids = torch.arange(x.shape[0])
        ref_of = lambda steps, nz, sm: _oracle64(monkeypatch, model, meta, x, steps, nz)
        return model, diff, x, ids, DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV), ref_of
    if name == "onehot_tiny":
        fx = H.load("onehot_sample_tiny_x0")
        meta = H.onehot_sample_meta(fx)
        I, dims = meta["I"], meta["dims"]
        model = gdmcf_amd.DNNOneHot([I] + dims, dims[::-1] + [I], 10)
        model.load_state_dict(H.state_dict_from(fx))
        om, od = H.oracle_onehot_pair(meta, fx)
        x = torch.from_numpy(fx["x_start"].astype(np.float32))
        ids = torch.arange(x.shape[0])
        ref_of = lambda steps, nz, sm: _oracle_discrete64(monkeypatch, om, od, x, steps, noise0=nz, sampled0=sm)
        return model.to(DEV).eval(), _discrete(meta), x, ids, DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV), ref_of
    if name == "emb_tiny":
        fx = H.load("onehot_emb_tiny_x0")
        meta = H.onehot_emb_meta(fx)
        I, dims, U = meta["I"], meta["dims"], meta["U"]
        model = gdmcf_amd.DNNOneHotEmbedding([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U)
        sd = H.state_dict_from(fx)
        sd.update(H.state_dict_from(fx, prefix="pN."))  # the fixture evaluates the weights after its training steps
        model.load_state_dict(sd)
        om, od = H.oracle_onehot_emb_pair(meta, fx)
        om.load_state_dict(sd)
        x, ids = torch.from_numpy(fx["e.x_start"].astype(np.float32)), torch.from_numpy(fx["e.index"]).long()
    else:
        assert name == "gcn_fresh"
        torch.manual_seed(13)
        I, U, T, dims = 131, 40, 5, [24]
        om = O.DNNOneHotEmbeddingGCN([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U, gcn_layers=2)
        with torch.no_grad():
            om.sumW.fill_(0.4)
            om.gcn_model.conv1.bias.normal_(0.0, 0.1)
            om.gcn_model.conv2.bias.normal_(0.0, 0.1)
        model = gdmcf_amd.DNNOneHotEmbeddingGCN([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U, gcn_layers=2)
        model.load_state_dict(om.state_dict())
        od = O.GaussianDiffusionDiscrete(O.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, CatOneHot=True)
        od.indexIn = True
        meta = dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99)
        x = _rows(10, I, 21)
        ids = torch.randperm(U, generator=torch.Generator().manual_seed(4))[:10]
    assert len(set(ids.tolist())) == len(ids)
    ref_of = lambda steps, nz, sm: _oracle_discrete64(monkeypatch, om, od, x, steps, noise0=nz, sampled0=sm, index=ids)
    return model.to(DEV).eval(), _discrete(meta, index_in=True), x, ids, _user_csr(x.numpy(), ids, U), ref_of


CASES = ["dnn_tiny", "dnn_ragged", "dnn_deep", "onehot_tiny", "emb_tiny", "gcn_fresh"]


@pytest.mark.parametrize("name", CASES)
def test_recommend_matches_the_float64_oracle(monkeypatch, name):
    model, diff, x, ids, dcsr, ref_of = _case(name, monkeypatch)
    B, I = x.shape
    T = diff.steps
    noise0, sampled0 = _draws(B, I)
    masked = x.numpy() != 0
    onehot = isinstance(diff, gdmcf_amd.GaussianDiffusionDiscrete)
    for steps, route in ((0, "latent-csr"), (T, "latent")):
        inj = {} if steps == 0 else (dict(noise0=noise0, sampled0=sampled0) if onehot else dict(noise0=noise0))
        ref = ref_of(steps, inj.get("noise0"), inj.get("sampled0"))
        for k in (1, 20):
            assert k <= I
            val, idx = recommend(diff, model, dcsr, ids, k, sampling_steps=steps, return_values=True, **inj)
            assert diff.last_recommend_route == route
            assert idx.dtype == torch.int64 and val.dtype == torch.float32 and idx.is_cuda
            _check_lists(val, idx, ref, masked, k, f"{name} steps={steps} k={k}")
            assert torch.equal(recommend(diff, model, dcsr, ids, k, sampling_steps=steps, **inj), idx)  # deterministic; ids alone


# ---------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------
def test_what_the_latent_routes_do_not_cover_gives_evaluates_bits():
    def same(diff, model, x, k=5, **kw):
        dcsr = DeviceCSR(sp.csr_matrix(x.astype(np.float64)), DEV)
        rows = np.arange(x.shape[0])
        val, idx = recommend(diff, model, dcsr, rows, k, return_values=True, **kw)
        assert diff.last_recommend_route == "item"
        pred = diff.p_sample(model, dcsr.rows(torch.from_numpy(rows)), kw.get("sampling_steps", 0), False)
        want = evaluate_utils.masked_topk(pred, k, *evaluate_utils.csr_rows_to_device(sp.csr_matrix(x), rows, DEV), return_values=True)
        assert torch.equal(idx, want[1]) and torch.equal(val, want[0])

    for case in ("ragged_eps", "norm_x0"):  # the eps target; F.normalize
        fx = H.load("sample_" + case)
        model, diff = dnn_pair(H.sample_meta(fx), fx)
        same(diff, model, fx["x_start"].astype(np.float32))
    fx = H.load("sample_ragged_x0")
    meta = H.sample_meta(fx)
    _, diff = dnn_pair(meta, fx)
    model16, _ = dnn_pair(meta, fx, gemm_dtype="bf16")  # bf16 products
    same(diff, model16, fx["x_start"].astype(np.float32))
    fx = H.load("dnncat_sample_tiny_x0")  # DNNCat
    meta = H.onehot_sample_meta(fx)
    I, dims = meta["I"], meta["dims"]
    cat = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], 10)
    cat.load_state_dict(H.state_dict_from(fx))
    same(_discrete(meta), cat.to(DEV).eval(), fx["x_start"].astype(np.float32))


@pytest.mark.parametrize("T", [3, 6])
@pytest.mark.parametrize("backbone", ["dnn", "onehot"])
def test_latent_csr_route_launches_no_builder_no_posterior_and_one_item_wide_product(monkeypatch, T, backbone):
    I, U, bs = 131, 10, 4
    x = _rows(U, I, 7)
    if backbone == "dnn":
        model, diff, _ = _fresh_dnn(I, [24], [24], T, seed=5)
    else:
        torch.manual_seed(5)
        model = gdmcf_amd.DNNOneHot([I, 24], [24, I], 10).to(DEV).eval()
        diff = _discrete(dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99))
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    eng = model.engine
    recommend(diff, model, dcsr, np.arange(U), 5, batch_size=bs)  # builds the cached operands (their own item-wide product)
    # the Philox position: as after p_sample(latent=True) on the same CsrBatch from the same start
    start = eng.offset
    diff.p_sample(model, dcsr.batch(torch.arange(bs)), 0, False, latent=True)
    assert diff.last_reverse_route == "latent"
    after_p_sample = eng.offset - start
    start = eng.offset
    recommend(diff, model, dcsr, np.arange(bs), 5, batch_size=bs)
    assert eng.offset - start == after_p_sample == 1
    calls = []

    def spy(mod, name, shape_of):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, **kw: (calls.append((name,) + shape_of(a)), real(*a, **kw))[1])

    spy(core, "linear_fwd", lambda a: (a[7], a[8]))            # (N, K)
    spy(core, "linear_bwd_input", lambda a: (a[8], a[9]))
    spy(core, "posterior_fwd", lambda a: ())
    spy(core, "prep_input_csr", lambda a: ())
    spy(core, "prep_input", lambda a: ())
    spy(core, "latent_step", lambda a: ())
    if hasattr(type(eng), "_prep_csr"):
        spy(type(eng), "_prep_csr", lambda a: ())
    spy(evaluate_utils, "csr_rows_to_device", lambda a: ())
    recommend(diff, model, dcsr, np.arange(U), 5, batch_size=bs)
    assert diff.last_recommend_route == "latent-csr"
    n_batches = -(-U // bs)
    names = [c[0] for c in calls]
    for gone in ("prep_input_csr", "_prep_csr", "prep_input", "posterior_fwd", "csr_rows_to_device", "linear_bwd_input"):
        assert gone not in names, gone
    item_wide = [c for c in calls if c[0] == "linear_fwd" and I in c[1:]]
    assert item_wide == [("linear_fwd", I, 24 if backbone == "dnn" else 48)] * n_batches  # one per batch, whatever T is
    assert names.count("latent_step") == (T - 1) * n_batches


def test_recommend_draws_the_graph_and_moves_the_counters_as_latent_p_sample():
    """recommend's docstring promise for an `indexIn` loop -- same draws, same `last_graph` as p_sample(latent=True) -- from the same
    engine offset and noise counter: on CSR rows ("latent-csr") and, with injected draws of x_T, on dense rows ("latent")."""
    I, U, T = 131, 10, 3
    torch.manual_seed(5)
    model = gdmcf_amd.DNNOneHotEmbedding([I, 24], [24, I], 10, item_num=I, user_num=U).to(DEV).eval()
    diff = _discrete(dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99), index_in=True)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    ids = cu(torch.randperm(U, generator=torch.Generator().manual_seed(2)))
    noise0, sampled0 = _draws(U, I)
    eng = model.engine

    def run(call):
        eng.offset, diff._noise_calls, diff.last_graph = 1000, 0, None
        call()
        return diff.last_graph.clone(), eng.offset - 1000, diff._noise_calls

    for steps, route, inj in ((0, "latent-csr", {}), (2, "latent", dict(noise0=cu(noise0), sampled0=cu(sampled0)))):
        rows = dcsr.batch(ids) if steps == 0 else dcsr.rows(ids)
        g_p, off_p, calls_p = run(lambda: diff.p_sample(model, rows, steps, False, index=ids, latent=True, **inj))
        assert diff.last_reverse_route == "latent"
        g_r, off_r, calls_r = run(lambda: recommend(diff, model, dcsr, ids, 5, batch_size=U, sampling_steps=steps, **inj))
        assert diff.last_recommend_route == route
        print(f"steps={steps}: graph bits {int(g_p.sum())} / {int(g_r.sum())}, offset +{off_p} / +{off_r}, noise calls {calls_p} / {calls_r}")
        assert bool(g_p.any()) and torch.equal(g_p, g_r)
        assert off_p == off_r and calls_p == calls_r == T


# ---------------------------------------------------------------------------------------------------------------------
# chunking and ids
# ---------------------------------------------------------------------------------------------------------------------
def test_chunks_permutations_and_repeats():
    I, U = 131, 10
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=5)
    dcsr = DeviceCSR(sp.csr_matrix(_rows(U, I, 7).numpy().astype(np.float64)), DEV)
    ids = torch.arange(U)
    val, idx = recommend(diff, model, dcsr, ids, 20, batch_size=400, return_values=True)
    val4, idx4 = recommend(diff, model, dcsr, ids, 20, batch_size=4, return_values=True)
    assert torch.equal(idx4, idx) and torch.equal(val4, val)
    perm = torch.randperm(U, generator=torch.Generator().manual_seed(1))
    assert torch.equal(recommend(diff, model, dcsr, perm, 20, batch_size=4), idx[perm.to(DEV)])
    rep = [3, 3, 9, 0, 3]
    assert torch.equal(recommend(diff, model, dcsr, rep, 20, batch_size=2), idx[torch.tensor(rep, device=DEV)])
    assert torch.equal(recommend(diff, model, dcsr, cu(perm), 20), idx[perm.to(DEV)])  # ids already on the device
    # mask: None ranks the history too; a second matrix removes its items as well
    free = recommend(diff, model, dcsr, ids, I, mask=None)
    assert bool((free.sort(dim=1).values == torch.arange(I, device=DEV)).all())
    other = DeviceCSR(sp.csr_matrix((np.random.default_rng(2).random((U, I)) < 0.3).astype(np.float64)), DEV)
    two = recommend(diff, model, dcsr, ids, 20, mask=(dcsr, other)).cpu().numpy()
    banned = (dcsr.rows(ids) != 0) | (other.rows(ids) != 0)
    assert not banned.cpu().numpy()[np.arange(U)[:, None], two].any()
    with pytest.raises(IndexError):
        recommend(diff, model, dcsr, [0, U], 5)
    assert recommend(diff, model, dcsr, [], 5).shape == (0, 5)


# ---------------------------------------------------------------------------------------------------------------------
# driver.evaluate(recommend=True)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone", ["dnn", "emb"])
def test_evaluate_recommend_gives_the_metrics_of_the_sparse_latent_evaluation(monkeypatch, backbone):
    U, I, bs, topN = 37, 131, 8, [5, 10]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    if backbone == "dnn":
        model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=2)
    else:
        torch.manual_seed(2)
        model = gdmcf_amd.DNNOneHotEmbedding([I, 24], [24, I], 10, item_num=I, user_num=U).to(DEV).eval()
        diff = _discrete(dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=5, discrete=0.99), index_in=True)
    want = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, sparse=True, latent=True)
    routes = []
    real = core.latent_step
    monkeypatch.setattr(evaluate_utils, "csr_rows_to_device", lambda *a: pytest.fail("host slicing on the recommend path"))
    monkeypatch.setattr(core, "latent_step", lambda *a: (routes.append((a[9], diff.last_recommend_route)), real(*a))[1])  # (a[9]: B)
    got = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, recommend=True)
    assert got == want, (got, want)
    assert [r for r in routes[::4]] == [(8, "latent-csr")] * 4 + [(5, "latent-csr")] and len(routes) == 4 * 5  # T - 1 steps a batch
    # a mask that already lives on the device is passed through
    assert driver.evaluate(diff, model, DeviceCSR(train, DEV), test, DeviceCSR(train, DEV), topN, 0, False, bs, DEV,
                           recommend=True) == want


# ---------------------------------------------------------------------------------------------------------------------
# freshness
# ---------------------------------------------------------------------------------------------------------------------
def test_lists_follow_an_eager_optimiser_step(monkeypatch):
    I, B, k = 131, 10, 20
    model, diff, meta = _fresh_dnn(I, [24], [24], 5, seed=4)
    x = _rows(B, I, 6)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    masked = x.numpy() != 0
    before = _oracle64(monkeypatch, model, meta, x)
    val, idx = recommend(diff, model, dcsr, np.arange(B), k, return_values=True)
    _check_lists(val, idx, before, masked, k, "before the step")
    ops = model.engine._latent[1]
    recommend(diff, model, dcsr, np.arange(B), k)
    assert model.engine._latent[1] is ops  # cached
    opt = torch.optim.Adam(model.parameters(), lr=0.02)  # (every weight moves by about lr, whatever the gradient's scale)
    model.train()
    model.drop.p = 0.0
    diff.training_losses(model, cu(x))["loss"].mean().backward()
    opt.step()
    model.eval()
    val2, idx2 = recommend(diff, model, dcsr, np.arange(B), k, return_values=True)
    assert diff.last_recommend_route == "latent-csr" and model.engine._latent[1] is not ops
    after = _oracle64(monkeypatch, model, meta, x)
    scale = max(np.abs(after).max(), 1.0)
    assert np.abs(after - before).max() > 100 * 2e-5 * scale  # the step really moved the result: stale operands cannot pass
    _check_lists(val2, idx2, after, masked, k, "after the step")
    assert not torch.equal(val2, val)
