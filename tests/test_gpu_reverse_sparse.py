"""GPU: the reverse loop from device CSR rows (sampling_steps == 0).  gdmcf_gather_fwd_f32 alone against float64 sums; `p_sample`
on a `CsrBatch` against the reference fixtures (DNN, DNNOneHot) and against the dense route (DNNOneHotEmbedding); what the
sparse route does not cover falls back to the dense route bit for bit; the one-hot route really skips the [B, 2I] image, xin2 and
the per-step branch-2 product; `driver.evaluate(sparse=True)`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import CsrBatch, DeviceCSR
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


def cu(t):
    return t.to(DEV)


def _mt(meta):
    return {"x0": ModelMeanType.START_X, "eps": ModelMeanType.EPSILON}[meta["mean_type"]]


def dnn_pair(meta, fx, **kw):
    I, dims = meta["I"], meta["dims"]
    m = gdmcf_amd.DNN([I] + dims, dims[::-1] + [I], 10, time_type="cat", norm=meta.get("norm", False), **kw)
    m.load_state_dict(H.state_dict_from(fx))
    d = gdmcf_amd.GaussianDiffusion(_mt(meta), "linear-var", meta["scale"], meta["nmin"], meta["nmax"], meta["T"], DEV).to(DEV)
    return m.to(DEV).eval(), d


def onehot_pair(meta, fx, cls=None):
    I, dims = meta["I"], meta["dims"]
    m = (cls or gdmcf_amd.DNNOneHot)([I] + dims, dims[::-1] + [I], 10)
    m.load_state_dict(H.state_dict_from(fx))
    d = gdmcf_amd.GaussianDiffusionDiscrete(_mt(meta), "linear-var", meta["scale"], meta["nmin"], meta["nmax"], meta["T"], DEV,
                                            discrete=meta["discrete"], CatOneHot=True)
    return m.to(DEV).eval(), d


def csr_batch(x, values=None):
    """All rows of the {0,1} array `x` as a CsrBatch on the device (values: replaces the stored ones)."""
    m = sp.csr_matrix(np.asarray(x, dtype=np.float64))
    if values is not None:
        m.data[:] = values
    return DeviceCSR(m, DEV).batch(torch.arange(x.shape[0]))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
KB, KI = 7, 515
# rows of the matrix: empty, one item, every item (two full index chunks and a remainder of 3), and lengths that are / are not
# multiples of the unroll factor 8, one of them just past an index chunk of 256; the batch takes seven of the nine in mixed order
ROW_NNZ = [0, 1, KI, 8, 13, 256 + 7, 60, 5, 256]
ROW_IDS = [2, 0, 8, 5, 1, 4, 3]
COMBOS = {"full": (1, 1, 1, 1), "layer1": (0, 0, 1, 1), "base_rows": (0, 1, 1, 0), "step": (1, 0, 0, 1)}  # pre, base, gather, bias


def _kernel_problem(N, E):
    g = torch.Generator().manual_seed(1000 * N + E)
    rng = np.random.default_rng(N + E)
    rows = [np.sort(rng.choice(KI, n, replace=False)) if n < KI else rng.permutation(KI) for n in ROW_NNZ]  # (one row unsorted)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    ldt = (N + 3) // 4 * 4 + 8
    p = dict(rows=rows, indptr=cu(torch.from_numpy(indptr)), indices=cu(torch.from_numpy(indices)),
             row_ids=cu(torch.tensor(ROW_IDS, dtype=torch.int64)), ldt=ldt)
    p["table"] = cu(torch.randn(KI, ldt, generator=g) * 0.05)
    p["tblE"] = cu(torch.randn(max(E, 1), ldt, generator=g) * 0.05)
    p["pre"] = cu(torch.randn(KB, N + 3, generator=g) * 0.3)  # (odd leading dimension: the scalar path of `pre`)
    p["base"], p["bias"] = cu(torch.randn(N, generator=g) * 0.3), cu(torch.randn(N, generator=g) * 0.01)
    p["a"] = cu(torch.randn(KB, E + 6, generator=g))
    return p


def _launch(p, N, E, combo, act, out):
    use_pre, use_base, use_rows, use_bias = COMBOS[combo]
    lib = _lib.load()
    _lib.check(lib.gdmcf_gather_fwd_f32(
        p["pre"].data_ptr() if use_pre else None, p["pre"].stride(0), p["base"].data_ptr() if use_base else None,
        p["indptr"].data_ptr() if use_rows else None, p["indices"].data_ptr() if use_rows else None,
        p["row_ids"].data_ptr() if use_rows else None, p["table"].data_ptr() if use_rows else None, p["ldt"], KI,
        p["a"].data_ptr() if E else None, p["a"].stride(0), p["tblE"].data_ptr() if E else None, p["ldt"], E,
        p["bias"].data_ptr() if use_bias else None, act, KB, N, out.data_ptr(), out.stride(0), _lib.stream_ptr()))
    return out


def _terms(p, N, E, combo):
    """(float64 pre-activation [B, N], per-element error bound of any float32 summation order): the terms of the sum as float64
    arrays, |err| <= (n_terms + 2) * 2^-24 * sum |terms| (recursive summation, first order, with two roundings to spare)."""
    use_pre, use_base, use_rows, use_bias = COMBOS[combo]
    tab, tE = p["table"].cpu().double().numpy()[:, :N], p["tblE"].cpu().double().numpy()[:, :N]
    s, sabs, nt = np.zeros((KB, N)), np.zeros((KB, N)), np.zeros((KB, 1))
    for b, r in enumerate(ROW_IDS):
        terms = []
        if use_pre:
            terms.append(p["pre"][b, :N].cpu().double().numpy())
        if use_base:
            terms.append(p["base"].cpu().double().numpy())
        if use_rows:
            terms += [tab[j] for j in p["rows"][r]]
        terms += [float(p["a"][b, e]) * tE[e] for e in range(E)]
        if use_bias:
            terms.append(p["bias"].cpu().double().numpy())
        if terms:
            s[b], sabs[b], nt[b] = np.sum(terms, axis=0), np.sum(np.abs(terms), axis=0), len(terms)
    return s, (nt + 2) * U24 * sabs


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("E", [0, 10])
@pytest.mark.parametrize("N", [5, 100, 1000, 1030])
def test_gather_kernel_matches_float64_sums(N, E, combo):
    """act = 0 within the recursive-summation bound; act = 1 within that bound (|tanh'| <= 1) plus twice the deviation of the
    existing gdmcf_linear_fwd_f32(act=1) from float64 tanh, measured here on the same sums written as a dense product
    [x | a] @ [table; tblE] (measured on the MI355X over all cases of this test: at most 1.76e-6, N = 1000 with E = 10, the 515-item row; this kernel with act = 1 deviates by at most 1.82e-6).  Two launches,
    and a launch into an output whose rows are not 16-byte aligned (the column range of hcat), give the same bits."""
    if combo == "step" and E == 0:
        combo = "full"  # (pre alone is not a layer: with E == 0 the fourth combination repeats the first on other sums)
    p = _kernel_problem(N, E)
    ref, bound = _terms(p, N, E, combo)
    ldo = (N + 3) // 4 * 4 + 4
    o0 = _launch(p, N, E, combo, 0, torch.full((KB, ldo), 7.0, device=DEV))
    err = np.abs(o0[:, :N].cpu().double().numpy() - ref)
    print(f"N={N} E={E} {combo}: act 0 max err {err.max():.3e}, smallest bound/err margin {(bound - err).min():.3e}")
    assert (err <= bound).all()
    assert bool((o0[:, N:] == 7.0).all())  # nothing is written behind column N
    # the same sums through the dense layer, as the yardstick of the tanh
    use_pre, use_base, use_rows, use_bias = COMBOS[combo]
    x = torch.zeros(KB, KI, device=DEV)
    if use_rows:
        for b, r in enumerate(ROW_IDS):
            x[b, torch.from_numpy(np.asarray(p["rows"][r], dtype=np.int64)).to(DEV)] = 1.0
    A = torch.cat([x, p["a"][:, :E]], dim=1).contiguous()
    W = torch.cat([p["table"][:, :N], p["tblE"][:E, :N]], dim=0).t().contiguous()
    bias_lin = (p["bias"] if use_bias else torch.zeros(N, device=DEV)).contiguous()
    lin = torch.empty(KB, N, device=DEV)
    ws_bytes = _lib.load().gdmcf_linear_ws_bytes(KB, N, KI + E)
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().gdmcf_linear_fwd_f32(A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), bias_lin.data_ptr(), 1, KB, N,
                                                KI + E, lin.data_ptr(), lin.stride(0), ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
    ref_lin = ref.copy()  # (the dense layer has no `pre` / `base` operand: take them out of its reference)
    if use_pre:
        ref_lin -= p["pre"][:, :N].cpu().double().numpy()
    if use_base:
        ref_lin -= p["base"].cpu().double().numpy()
    dev_lin = np.abs(lin.cpu().double().numpy() - np.tanh(ref_lin)).max()
    o1 = _launch(p, N, E, combo, 1, torch.full((KB, ldo), 7.0, device=DEV))
    err1 = np.abs(o1[:, :N].cpu().double().numpy() - np.tanh(ref))
    print(f"N={N} E={E} {combo}: act 1 max err {err1.max():.3e}; gdmcf_linear_fwd_f32(act=1) deviates {dev_lin:.3e} from float64 tanh")
    assert (err1 <= bound + 2 * dev_lin).all()
    # determinism and the unaligned output
    for act, first in ((0, o0), (1, o1)):
        again = _launch(p, N, E, combo, act, torch.full((KB, ldo), 7.0, device=DEV))
        assert torch.equal(again, first)
        shifted = torch.full((KB, ldo + 4), 7.0, device=DEV)
        _launch(p, N, E, combo, act, shifted[:, 1:])
        assert torch.equal(shifted[:, 1:1 + N], first[:, :N])
        assert bool((shifted[:, 0] == 7.0).all()) and bool((shifted[:, 1 + N:] == 7.0).all())


def test_gather_kernel_skips_indices_outside_the_table():
    """The same rows over a table declared two items shorter: the entries for items 513 and 514 drop out of the sums."""
    N = 100
    p = _kernel_problem(N, 0)
    out = torch.zeros(KB, 104, device=DEV)
    _lib.check(_lib.load().gdmcf_gather_fwd_f32(
        None, 0, None, p["indptr"].data_ptr(), p["indices"].data_ptr(), p["row_ids"].data_ptr(), p["table"].data_ptr(), p["ldt"],
        KI - 2, None, 0, None, 0, 0, p["bias"].data_ptr(), 0, KB, N, out.data_ptr(), out.stride(0), _lib.stream_ptr()))
    tab, bias = p["table"].cpu().double().numpy()[:, :N], p["bias"].cpu().double().numpy()
    for b, r in enumerate(ROW_IDS):
        terms = [tab[j] for j in p["rows"][r] if j < KI - 2] + [bias]
        bound = (len(terms) + 2) * U24 * np.sum(np.abs(terms), axis=0)
        assert (np.abs(out[b, :N].cpu().double().numpy() - np.sum(terms, axis=0)) <= bound).all(), b


# ---------------------------------------------------------------------------------------------------------------------
# DNN against the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_x0", "ragged_x0", "ragged_eps"])
def test_dnn_p_sample_from_csr_rows_matches_reference(case):
    fx = H.load("sample_" + case)
    meta = H.sample_meta(fx)
    model, diff = dnn_pair(meta, fx)
    T, k = meta["T"], meta["k"]
    batch = csr_batch(fx["x_start"])
    assert diff._sparse_reverse_ok(model, batch, 0)
    cap = {}
    p0 = diff.p_sample(model, batch, 0, False, capture=cap)
    scale = np.abs(fx["pred_steps0"]).max()
    assert np.abs(p0.cpu().numpy() - fx["pred_steps0"]).max() < 2e-5 * max(scale, 1.0)
    for n in range(T):
        assert H.relerr(cap["pred_xstart"][n].cpu().numpy(), fx["step_pred_xstart"][n]) < 2e-5
        assert H.relerr(cap["mean"][n].cpu().numpy(), fx["step_mean"][n]) < 2e-5
    his = torch.from_numpy(fx["x_start"].astype(np.float32)).to_sparse_csr()
    idx = gdmcf_amd.masked_topk(p0, k, his.crow_indices(), his.col_indices()).cpu().numpy()
    tol = 1e-4 * max(scale, 1.0)
    for b in range(meta["B"]):
        if fx["topk_gap"][b] > tol:
            assert set(idx[b].tolist()) == set(fx["topk_idx"][b].tolist()), b
        if fx["topk_min_adjacent_gap"][b] > tol:
            np.testing.assert_array_equal(idx[b], fx["topk_idx"][b])
    # the route is deterministic
    assert torch.equal(diff.p_sample(model, batch, 0, False), p0)


# ---------------------------------------------------------------------------------------------------------------------
# one-hot family
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.ONEHOT_SAMPLE_CASES)
def test_onehot_p_sample_from_csr_rows_matches_reference(case):
    fx = H.load("onehot_sample_" + case)
    meta = H.onehot_sample_meta(fx)
    model, diff = onehot_pair(meta, fx)
    batch = csr_batch(fx["x_start"])
    p0 = diff.p_sample(model, batch, 0, False)
    assert H.relerr(p0.cpu().numpy(), fx["pred_steps0"]) < 2e-5
    assert torch.equal(diff.p_sample(model, batch, 0, False), p0)


def _emb_pair(dims, I=131, U=40, T=5, mean_type=ModelMeanType.START_X):
    torch.manual_seed(11 + len(dims))
    m = gdmcf_amd.DNNOneHotEmbedding([I] + list(dims), list(dims)[::-1] + [I], 10, item_num=I, user_num=U).to(DEV).eval()
    d = gdmcf_amd.GaussianDiffusionDiscrete(mean_type, "linear-var", 0.01, 0.001, 0.01, T, DEV, discrete=0.99, CatOneHot=True)
    d.indexIn = True
    return m, d


@pytest.mark.parametrize("dims", [(24,), (32, 24)])
def test_onehot_embedding_sparse_route_matches_dense_route(dims):
    """Fresh weights, one and two layers per branch (a deeper in_layers2 layer behind the hoisted one), users in random order.
    Either route is within 2e-5 of the reference (the project's bound for this backbone's reverse loop): 4e-5 between them."""
    I, B = 131, 10
    model, diff = _emb_pair(dims, I)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, I, generator=g) < 0.15).float()
    x[3] = 0.0
    index = torch.randperm(40, generator=g)[:B]
    cap_d, cap_s = {}, {}
    diff._noise_calls = 0
    dense = diff.p_sample(model, cu(x), 0, False, index=index, capture=cap_d)
    diff._noise_calls = 0  # (the graph draws are counted per diffusion object: the second loop repeats the first one's)
    sparse = diff.p_sample(model, csr_batch(x.numpy()), 0, False, index=index, capture=cap_s)
    assert H.relerr(sparse.cpu().numpy(), dense.cpu().numpy()) < 4e-5
    for n in range(5):
        assert H.relerr(cap_s["pred_xstart"][n].cpu().numpy(), cap_d["pred_xstart"][n].cpu().numpy()) < 4e-5
        assert torch.equal(cap_s["graph"][n], cap_d["graph"][n])  # (the degree probabilities come from indptr: same draws)


# ---------------------------------------------------------------------------------------------------------------------
# fallbacks: the dense route's bits
# ---------------------------------------------------------------------------------------------------------------------
def test_what_the_sparse_route_does_not_cover_runs_the_dense_route():
    # F.normalize
    fx = H.load("sample_norm_x0")
    meta = H.sample_meta(fx)
    model, diff = dnn_pair(meta, fx)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    batch = csr_batch(fx["x_start"])
    assert model.norm and not diff._sparse_reverse_ok(model, batch, 0)
    assert torch.equal(diff.p_sample(model, batch, 0, False), diff.p_sample(model, x, 0, False))
    # steps = T with the noise given; bf16 products; a value other than 1
    fx = H.load("sample_ragged_x0")
    meta = H.sample_meta(fx)
    model, diff = dnn_pair(meta, fx)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    batch = csr_batch(fx["x_start"])
    noise0 = cu(torch.from_numpy(fx["noise_stepsT"]))
    assert torch.equal(diff.p_sample(model, batch, meta["T"], False, noise0=noise0), diff.p_sample(model, x, meta["T"], False, noise0=noise0))
    model16, _ = dnn_pair(meta, fx, gemm_dtype="bf16")
    assert torch.equal(diff.p_sample(model16, batch, 0, False), diff.p_sample(model16, x, 0, False))
    valued = csr_batch(fx["x_start"], values=2.0)
    assert valued.csr.values is not None
    assert torch.equal(diff.p_sample(model, valued, 0, False), diff.p_sample(model, 2.0 * x, 0, False))
    # DNNCat
    fx = H.load("dnncat_sample_tiny_x0")
    meta = H.onehot_sample_meta(fx)
    model, diff = onehot_pair(meta, fx, cls=gdmcf_amd.DNNCat)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    assert torch.equal(diff.p_sample(model, csr_batch(fx["x_start"]), 0, False), diff.p_sample(model, x, 0, False))


# ---------------------------------------------------------------------------------------------------------------------
# the route is really taken
# ---------------------------------------------------------------------------------------------------------------------
def test_onehot_sparse_route_builds_no_image_no_xin2_and_gathers_branch2_once(monkeypatch):
    fx = H.load("onehot_sample_ragged_eps")
    meta = H.onehot_sample_meta(fx)
    model, diff = onehot_pair(meta, fx)
    eng = model.engine
    widths, gathers = [], []
    real_prep = eng._prep_input
    monkeypatch.setattr(eng, "_prep_input", lambda bufs, x, I, *a, **kw: (widths.append(I), real_prep(bufs, x, I, *a, **kw))[1])
    real_gather = core.gather_fwd
    monkeypatch.setattr(core, "gather_fwd", lambda lib_, pre, base, batch, *a: (gathers.append((pre is not None, base is not None,
                                                                                               batch is not None)),
                                                                                real_gather(lib_, pre, base, batch, *a))[1])
    diff.p_sample(model, csr_batch(fx["x_start"]), 0, False)
    T, bufs = meta["T"], eng.buffers(meta["B"], torch.device(DEV))
    assert bufs.xU is None and "xin2" not in vars(bufs)
    assert widths == [meta["I"]] * (T - 1)  # branch 1's dense builder from the second step on; never the 2I-wide one
    # (pre, base, rows): branch 2's rows once per loop with base = S0; branch 1's rows at the first step; branch 2 from P2 per step
    assert gathers.count((False, True, True)) == 1 and gathers.count((False, False, True)) == 1
    assert gathers.count((True, False, False)) == T and len(gathers) == T + 2
    assert eng.sparse_gathers == 1
    # the dense route on the same engine still builds xin2 from the image, once per step
    diff.p_sample(model, cu(torch.from_numpy(fx["x_start"].astype(np.float32))), 0, False)
    assert "xin2" in vars(bufs) and widths.count(2 * meta["I"]) == T


# ---------------------------------------------------------------------------------------------------------------------
# driver.evaluate(sparse=True)
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_sparse_hands_csr_batches_and_reproduces_its_own_loop(monkeypatch):
    U, I, bs, topN = 25, 131, 8, [5, 10]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    torch.manual_seed(2)
    model = gdmcf_amd.DNN([I, 24], [24, I], 10, time_type="cat").to(DEV).eval()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, DEV).to(DEV)
    seen = []
    real = diff.p_sample
    monkeypatch.setattr(diff, "p_sample", lambda m, b, *a, **kw: (seen.append(b), real(m, b, *a, **kw))[1])
    got = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, sparse=True)
    assert len(seen) == 4 and all(isinstance(b, CsrBatch) for b in seen) and [b.shape[0] for b in seen] == [8, 8, 8, 1]
    dcsr, lists = DeviceCSR(train, DEV), []
    for lo in range(0, U, bs):
        rows = np.arange(lo, min(lo + bs, U))
        pred = real(model, dcsr.batch(torch.from_numpy(rows)), 0, False)
        indptr, cols = gdmcf_amd.evaluate_utils.csr_rows_to_device(train, rows, DEV)
        lists.append(gdmcf_amd.masked_topk(pred, topN[-1], indptr, cols))
    want = gdmcf_amd.evaluate_utils.computeTopNAccuracy_device(test, torch.cat(lists), topN)
    assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
