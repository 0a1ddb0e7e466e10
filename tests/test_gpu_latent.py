"""GPU: the reverse loop carried in the first hidden layer's space (`p_sample(latent=True)`).
gdmcf_latent_step_f32 alone against a float64 product of the same formula, every element, within a derived bound; the DNN loop
against the reference fixtures (dense rows and CSR rows, steps = 0 and steps = T) and, for a deep DNN, against the CPU oracle in
float64; what the latent route does not cover takes the item-space route bit for bit; the cached operands follow the weights
(eager optimiser steps, hipGraph replays); the loop really makes two item-wide products whatever T is; `driver.evaluate(latent=True)`."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib, driver
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import DeviceCSR
from oracle import gdmcf_oracle as O
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


def csr_batch(x):
    return DeviceCSR(sp.csr_matrix(np.asarray(x, dtype=np.float64)), DEV).batch(torch.arange(x.shape[0]))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 16, 16), (7, 24, 50), (37, 100, 97), (129, 1000, 257), (400, 1000, 1000), (64, 1000, 3000)]
# (v, e, act, h_next, p_next aliases p_cur)
OPTIONS = {"full": (1, 1, 1, 1, 0), "bare": (0, 0, 0, 1, 0), "no_h_alias": (1, 0, 1, 0, 1), "e_only_alias": (0, 1, 1, 1, 1),
           "v_only_linear": (1, 0, 0, 1, 0)}


def _pad(n, odd):
    """A leading dimension for rows of n elements: 16-byte aligned rows (a multiple of 4 with room to spare), or an odd one (rows
    that are not 16-byte aligned: the kernel's scalar paths)."""
    return n + 1 + (n % 2) if odd else (n + 3) // 4 * 4 + 8


_PROBLEMS = {}


def _problem(B, N, K, odd):
    """Operands on the device and the float64 reference terms, computed once per (shape, leading dimensions) and never modified."""
    key = (B, N, K, odd)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(7 * B + 11 * N + 13 * K + odd)
    A = torch.tanh(torch.randn(B, _pad(K, odd), generator=g))            # activations: |a| < 1
    M = torch.randn(N, _pad(K, odd), generator=g) * (2.0 / K ** 0.5)
    v = torch.randn(N, generator=g) * 0.3
    e = torch.randn(N, generator=g) * 0.3
    pc = torch.randn(B, _pad(N, odd), generator=g)
    c1 = torch.rand(B, generator=g) * 0.9 + 0.1
    c2 = torch.rand(B, generator=g) * 0.9
    c2[::3] = 0.0                                                        # rows whose posterior has no x_t term (the last step's)
    A64, M64 = A[:, :K].double(), M[:, :K].double()
    p = dict(A=cu(A), M=cu(M), v=cu(v), e=cu(e), pc=cu(pc), c1=cu(c1), c2=cu(c2), s=A64 @ M64.t(), sabs=A64.abs() @ M64.abs().t(),
             v64=v.double(), e64=e.double(), pc64=pc[:, :N].double(), c164=c1.double()[:, None], c264=c2.double()[:, None])
    _PROBLEMS[key] = p
    return p


def _reference(p, K, use_v, use_e, act):
    """float64 (p_next, h_next) and their per-element bounds.  Linear part, u = 2^-24: the K products are summed by fma chains
    and three additions of partial sums (at most K roundings on a path, each relative to a partial sum of |A M|), then one
    rounding each for + v, for c1 *, and for the fma with c2 p_cur: |err p_next| <= (K + 6) u (|c1| (sum |A M| + |v|) + |c2| |p_cur|)
    to first order, with roundings to spare.  Activation: |tanh'| <= 1 carries that bound over; the sum p_next + e adds one
    rounding of at most u (|p_next| + |e|) -- the |p_next| part is inside the spare roundings above -- and tanhf is within 2 ulp of
    a result below 1: 4 u."""
    vv = p["v64"] if use_v else torch.zeros_like(p["v64"])
    pn = p["c164"] * (p["s"] + vv) + p["c264"] * p["pc64"]
    bp = (K + 6) * U24 * (p["c164"].abs() * (p["sabs"] + vv.abs()) + p["c264"].abs() * p["pc64"].abs())
    z = pn + (p["e64"] if use_e else 0.0)
    h = torch.tanh(z) if act == 1 else z
    bh = bp + U24 * (p["e64"].abs() if use_e else 0.0) + 4 * U24
    return pn, bp, h, bh


def _launch(p, B, N, K, odd, opt, p_cur=None):
    use_v, use_e, act, use_h, alias = OPTIONS[opt]
    lib = _lib.load()
    pc = (p["pc"] if p_cur is None else p_cur).clone()
    pn = pc if alias else torch.full((B, _pad(N, odd) + 4), 7.0, device=DEV)
    h = torch.full((B, _pad(N, odd) + 8), 7.0, device=DEV) if use_h else None
    assert lib.gdmcf_latent_step_ws_bytes(B, N, K) == 0
    _lib.check(lib.gdmcf_latent_step_f32(
        p["A"].data_ptr(), p["A"].stride(0), p["M"].data_ptr(), p["M"].stride(0), p["v"].data_ptr() if use_v else None,
        pc.data_ptr(), pc.stride(0), p["c1"].data_ptr(), p["c2"].data_ptr(), p["e"].data_ptr() if use_e else None, act, B, N, K,
        pn.data_ptr(), pn.stride(0), h.data_ptr() if use_h else None, h.stride(0) if use_h else 0, None, 0, _lib.stream_ptr()))
    return pn, h


def _check_kernel(B, N, K, odd):
    p = _problem(B, N, K, odd)
    for opt, (use_v, use_e, act, use_h, alias) in OPTIONS.items():
        ref_p, bound_p, ref_h, bound_h = _reference(p, K, use_v, use_e, act)
        pn, h = _launch(p, B, N, K, odd, opt)
        err = (pn[:, :N].cpu().double() - ref_p).abs()
        print(f"B={B} N={N} K={K} odd={odd} {opt}: p_next max err {float(err.max()):.3e}, largest err/bound "
              f"{float((err / bound_p.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound_p).all())
        if alias:
            assert torch.equal(pn[:, N:], p["pc"][:, N:])  # nothing is written behind column N
        else:
            assert bool((pn[:, N:] == 7.0).all())
        if use_h:
            errh = (h[:, :N].cpu().double() - ref_h).abs()
            print(f"    h_next max err {float(errh.max()):.3e}, largest err/bound {float((errh / bound_h).max()):.3f}")
            assert bool((errh <= bound_h).all()) and bool((h[:, N:] == 7.0).all())
        pn2, h2 = _launch(p, B, N, K, odd, opt)  # the same bits on every run
        assert torch.equal(pn2, pn) and (h is None or torch.equal(h2, h))
    # a row with c2 == 0 does not read p_cur (documented at the declaration): poison those rows
    poisoned = p["pc"].clone()
    poisoned[::3] = float("nan")
    ref_p, bound_p, _, _ = _reference(p, K, 1, 1, 1)
    pn, h = _launch(p, B, N, K, odd, "full", p_cur=poisoned)
    assert bool(((pn[:, :N].cpu().double() - ref_p).abs() <= bound_p).all()) and bool(torch.isfinite(h[:, :N]).all())


@pytest.mark.parametrize("B,N,K", SHAPES)
def test_latent_step_kernel_matches_float64_product(B, N, K):
    """Rows of A, M, p_cur, p_next and h_next on 16-byte boundaries with padded leading dimensions: whole chunks by 16-byte loads,
    the last partial chunk (K = 50, 97, 257, 1000, 3000 are no multiples of 16) by guarded ones; B and N tails of the 16 x 64 tile."""
    _check_kernel(B, N, K, 0)


@pytest.mark.parametrize("B,N,K", [(7, 24, 50), (37, 100, 97), (129, 1000, 257)])
def test_latent_step_kernel_with_odd_leading_dimensions(B, N, K):
    """Every leading dimension odd: no row but the first is 16-byte aligned -- scalar loads and stores throughout."""
    _check_kernel(B, N, K, 1)


def test_latent_step_kernel_is_capture_safe():
    """No host synchronisation, no allocation: the launch can be captured and replayed."""
    B, N, K = 37, 100, 97
    p = _problem(B, N, K, 0)
    want, want_h = _launch(p, B, N, K, 0, "full")
    pn, h = torch.zeros_like(want), torch.zeros_like(want_h)
    lib, pc = _lib.load(), p["pc"]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.gdmcf_latent_step_f32(
            p["A"].data_ptr(), p["A"].stride(0), p["M"].data_ptr(), p["M"].stride(0), p["v"].data_ptr(), pc.data_ptr(),
            pc.stride(0), p["c1"].data_ptr(), p["c2"].data_ptr(), p["e"].data_ptr(), 1, B, N, K, pn.data_ptr(), pn.stride(0),
            h.data_ptr(), h.stride(0), None, 0, _lib.stream_ptr()))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(pn[:, :N], want[:, :N]) and torch.equal(h[:, :N], want_h[:, :N])


# ---------------------------------------------------------------------------------------------------------------------
# DNN against the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _check_topk(fx, meta, pred):
    scale = np.abs(fx["pred_steps0"]).max()
    his = torch.from_numpy(fx["x_start"].astype(np.float32)).to_sparse_csr()
    idx = gdmcf_amd.masked_topk(pred, meta["k"], his.crow_indices(), his.col_indices()).cpu().numpy()
    tol = 1e-4 * max(scale, 1.0)
    assert bool((fx["topk_gap"] > tol).all())  # every row of the fixture takes part
    for b in range(meta["B"]):
        assert set(idx[b].tolist()) == set(fx["topk_idx"][b].tolist()), b


@pytest.mark.parametrize("case", ["tiny_x0", "ragged_x0"])
def test_dnn_latent_p_sample_matches_reference(case):
    fx = H.load("sample_" + case)
    meta = H.sample_meta(fx)
    model, diff = dnn_pair(meta, fx)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    scale = np.abs(fx["pred_steps0"]).max()
    for rows in (x, csr_batch(fx["x_start"])):
        p0 = diff.p_sample(model, rows, 0, False, latent=True)
        assert diff.last_reverse_route == "latent"
        dev = np.abs(p0.cpu().numpy() - fx["pred_steps0"]).max()
        print(f"{case} steps=0 {type(rows).__name__}: deviation {dev:.3e} of scale {scale:.3e}")
        assert p0.dtype == torch.float32 and tuple(p0.shape) == (meta["B"], meta["I"])
        assert dev < 2e-5 * max(scale, 1.0)
        _check_topk(fx, meta, p0)
        assert torch.equal(diff.p_sample(model, rows, 0, False, latent=True), p0)  # the route is deterministic
    T = meta["T"]
    pT = diff.p_sample(model, x, T, False, noise0=cu(torch.from_numpy(fx["noise_stepsT"])), latent=True)
    assert diff.last_reverse_route == "latent"
    scaleT = np.abs(fx["pred_stepsT"]).max()
    devT = np.abs(pT.cpu().numpy() - fx["pred_stepsT"]).max()
    print(f"{case} steps=T: deviation {devT:.3e} of scale {scaleT:.3e}")
    assert devT < 2e-5 * max(scaleT, 1.0)
    # CSR rows with steps = T are densified (x_T is no longer binary) and still take the latent route
    pT_csr = diff.p_sample(model, csr_batch(fx["x_start"]), T, False, noise0=cu(torch.from_numpy(fx["noise_stepsT"])), latent=True)
    assert diff.last_reverse_route == "latent" and torch.equal(pT_csr, pT)
    # the default is untouched
    diff.p_sample(model, x, 0, False)
    assert diff.last_reverse_route == "item"


def _oracle64(monkeypatch, model, meta, x, steps=0, noise0=None):
    """The CPU oracle in float64 on the device model's current state dict."""
    real = O.timestep_embedding
    monkeypatch.setattr(O, "timestep_embedding", lambda t, d, *a: real(t, d, *a).double())
    I, dims_in, dims_out = meta["I"], meta["dims_in"], meta["dims_out"]
    om = O.DNN([I] + dims_in, dims_out + [I], 10)
    om.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    om = om.double().eval()
    od = O.GaussianDiffusion(O.ModelMeanType.START_X, "linear-var", meta["scale"], meta["nmin"], meta["nmax"], meta["T"])
    with torch.no_grad():
        return od.p_sample(om, x.cpu().double(), steps, False, noise0=None if noise0 is None else noise0.cpu().double()).numpy()


def _fresh_dnn(I, dims_in, dims_out, T, seed, scale=0.01):
    torch.manual_seed(seed)
    model = gdmcf_amd.DNN([I] + dims_in, dims_out + [I], 10, time_type="cat").to(DEV).eval()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", scale, 0.001, 0.01, T, DEV).to(DEV)
    meta = dict(I=I, dims_in=dims_in, dims_out=dims_out, T=T, scale=scale, nmin=0.001, nmax=0.01)
    return model, diff, meta


def _rows(B, I, seed, density=0.12):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, I, generator=g) < density).float()
    x[min(3, B - 1)] = 0.0  # an empty row
    return x


def test_deep_dnn_latent_matches_float64_oracle(monkeypatch):
    """dims = [24, 40]: two layers on either side, so that hidden layers run between the step kernel's h_next and its operand A."""
    I, B = 131, 10
    model, diff, meta = _fresh_dnn(I, [24, 40], [40, 24], 5, seed=3)
    x = _rows(B, I, 1)
    g = torch.Generator().manual_seed(2)
    noise0 = torch.randn(B, I, generator=g)
    for steps, nz, rows in ((0, None, cu(x)), (0, None, csr_batch(x.numpy())), (5, noise0, cu(x))):
        ref = _oracle64(monkeypatch, model, meta, x, steps, nz)
        got = diff.p_sample(model, rows, steps, False, noise0=None if nz is None else cu(nz), latent=True)
        assert diff.last_reverse_route == "latent"
        scale = np.abs(ref).max()
        dev = np.abs(got.cpu().double().numpy() - ref).max()
        print(f"deep DNN steps={steps} {type(rows).__name__}: deviation {dev:.3e} of scale {scale:.3e}")
        assert dev < 2e-5 * max(scale, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the one-hot backbones: the fixture where one exists, otherwise the CPU oracle in float64
# ---------------------------------------------------------------------------------------------------------------------
def _discrete(meta, index_in=False):
    d = gdmcf_amd.GaussianDiffusionDiscrete(_mt(meta), meta.get("schedule", "linear-var"), meta["scale"], meta["nmin"], meta["nmax"],
                                            meta["T"], DEV, discrete=meta["discrete"], CatOneHot=True)
    d.indexIn = index_in
    return d


def _within(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    dev = np.abs(got.cpu().double().numpy() - ref).max()
    print(f"{what}: deviation {dev:.3e} of scale {scale:.3e}")
    assert got.dtype == torch.float32 and got.shape == ref.shape
    assert dev < 2e-5 * max(scale, 1.0)


def _oracle_discrete64(monkeypatch, om, od, x, steps, noise0=None, sampled0=None, index=None):
    real = O.timestep_embedding
    monkeypatch.setattr(O, "timestep_embedding", lambda t, d, *a: real(t, d, *a).double())
    om = om.double().eval()
    with torch.no_grad():
        return od.p_sample(om, x.double(), steps, False, noise0=None if noise0 is None else noise0.double(), sampled0=sampled0,
                           index=index).numpy()


def _latent_cases(monkeypatch, model, diff, x, ref_of, index=None):
    """steps = 0 from dense rows and from CSR rows, steps = T from dense rows with injected draws; the graph of an indexIn loop is
    the item-space route's, draw for draw."""
    B, I = x.shape
    T = diff.steps
    g = torch.Generator().manual_seed(17)
    noise0, sampled0 = torch.randn(B, I, generator=g), (torch.rand(B, I, generator=g) < 0.1).long()
    kw = dict(index=index) if index is not None else {}
    for steps, rows, inj in ((0, cu(x), {}), (0, csr_batch(x.numpy()), {}), (T, cu(x), dict(noise0=noise0, sampled0=sampled0))):
        diff._noise_calls = 0
        got = diff.p_sample(model, rows, steps, False, latent=True, **kw, **{k: cu(v) for k, v in inj.items()})
        assert diff.last_reverse_route == "latent"
        graph = diff.last_graph
        _within(got, ref_of(steps, inj), f"{type(model).__name__} steps={steps} {type(rows).__name__}")
        if index is not None:
            diff._noise_calls = 0
            diff.p_sample(model, rows, steps, False, **kw, **{k: cu(v) for k, v in inj.items()})
            assert diff.last_reverse_route == "item" and graph is not None and torch.equal(diff.last_graph, graph)


def test_onehot_latent_matches_reference_fixture():
    fx = H.load("onehot_sample_tiny_x0")
    meta = H.onehot_sample_meta(fx)
    I, dims = meta["I"], meta["dims"]
    model = gdmcf_amd.DNNOneHot([I] + dims, dims[::-1] + [I], 10)
    model.load_state_dict(H.state_dict_from(fx))
    model, diff = model.to(DEV).eval(), _discrete(meta)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    for rows in (x, csr_batch(fx["x_start"])):
        p0 = diff.p_sample(model, rows, 0, False, latent=True)
        assert diff.last_reverse_route == "latent"
        _within(p0, fx["pred_steps0"], f"DNNOneHot fixture steps=0 {type(rows).__name__}")
    pT = diff.p_sample(model, x, meta["T"], False, noise0=cu(torch.from_numpy(fx["noise_stepsT"])),
                       sampled0=cu(torch.from_numpy(fx["sampled_stepsT"])), latent=True)
    assert diff.last_reverse_route == "latent"
    _within(pT, fx["pred_stepsT"], "DNNOneHot fixture steps=T")


def test_onehot_latent_matches_float64_oracle(monkeypatch):
    """The weights of onehot_sample_ragged_eps (B = 10, I = 131) run under the x0 target."""
    fx = H.load("onehot_sample_ragged_eps")
    meta = dict(H.onehot_sample_meta(fx), mean_type="x0")
    I, dims = meta["I"], meta["dims"]
    model = gdmcf_amd.DNNOneHot([I] + dims, dims[::-1] + [I], 10)
    model.load_state_dict(H.state_dict_from(fx))
    model, diff = model.to(DEV).eval(), _discrete(meta)
    om, od = H.oracle_onehot_pair(meta, fx)
    x = torch.from_numpy(fx["x_start"].astype(np.float32))
    _latent_cases(monkeypatch, model, diff, x, lambda steps, inj: _oracle_discrete64(monkeypatch, om, od, x, steps, **inj))


def test_onehot_embedding_latent_matches_reference_fixture():
    """The fixture's evaluation runs on the weights after its two training steps (pN.*)."""
    fx = H.load("onehot_emb_tiny_x0")
    meta = H.onehot_emb_meta(fx)
    I, dims = meta["I"], meta["dims"]
    model = gdmcf_amd.DNNOneHotEmbedding([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=meta["U"])
    sd = H.state_dict_from(fx)
    sd.update(H.state_dict_from(fx, prefix="pN."))
    model.load_state_dict(sd)
    model, diff = model.to(DEV).eval(), _discrete(meta, index_in=True)
    x, idx = cu(torch.from_numpy(fx["e.x_start"].astype(np.float32))), torch.from_numpy(fx["e.index"])
    for rows in (x, csr_batch(fx["e.x_start"])):
        p0 = diff.p_sample(model, rows, 0, False, index=idx, latent=True)
        assert diff.last_reverse_route == "latent"
        _within(p0, fx["e.pred_steps0"], f"DNNOneHotEmbedding fixture steps=0 {type(rows).__name__}")
    pT = diff.p_sample(model, x, meta["T"], False, index=idx, noise0=cu(torch.from_numpy(fx["e.noise_stepsT"])),
                       sampled0=cu(torch.from_numpy(fx["e.sampled_stepsT"])), latent=True)
    assert diff.last_reverse_route == "latent"
    _within(pT, fx["e.pred_stepsT"], "DNNOneHotEmbedding fixture steps=T")


@pytest.mark.parametrize("backbone,dims", [("emb", (32, 24)), ("gcn", (24,))])
def test_embedding_backbones_latent_match_float64_oracle(monkeypatch, backbone, dims):
    """Fresh weights: the embedding backbone with two layers per branch (small layers between the step kernel's h_next and the
    scored vector), and the GCN backbone with sumW away from 1 so that its perceptron carries weight."""
    torch.manual_seed(13)
    I, B, T, U = 131, 10, 5, 40
    dims = list(dims)
    if backbone == "gcn":
        om = O.DNNOneHotEmbeddingGCN([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U, gcn_layers=2)
        with torch.no_grad():
            om.sumW.fill_(0.4)
            om.gcn_model.conv1.bias.normal_(0.0, 0.1)
            om.gcn_model.conv2.bias.normal_(0.0, 0.1)
        gm = gdmcf_amd.DNNOneHotEmbeddingGCN([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U, gcn_layers=2)
    else:
        om = O.DNNOneHotEmbedding([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U)
        gm = gdmcf_amd.DNNOneHotEmbedding([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=U)
    gm.load_state_dict(om.state_dict())
    gm = gm.to(DEV).eval()
    od = O.GaussianDiffusionDiscrete(O.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, CatOneHot=True)
    od.indexIn = True
    meta = dict(mean_type="x0", scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99)
    diff = _discrete(meta, index_in=True)
    x = _rows(B, I, 21)
    index = torch.randperm(U, generator=torch.Generator().manual_seed(4))[:B]
    _latent_cases(monkeypatch, gm, diff, x, lambda steps, inj: _oracle_discrete64(monkeypatch, om, od, x, steps, index=index, **inj),
                  index=index)


# ---------------------------------------------------------------------------------------------------------------------
# fallbacks: the item-space route's bits
# ---------------------------------------------------------------------------------------------------------------------
def test_what_the_latent_route_does_not_cover_runs_the_item_route():
    def same(diff, model, *a, **kw):
        item = diff.p_sample(model, *a, **kw)
        assert diff.last_reverse_route == "item"
        lat = diff.p_sample(model, *a, latent=True, **kw)
        assert diff.last_reverse_route == "item"
        assert torch.equal(lat, item)

    for case in ("ragged_eps", "norm_x0"):  # the eps target; F.normalize
        fx = H.load("sample_" + case)
        meta = H.sample_meta(fx)
        model, diff = dnn_pair(meta, fx)
        same(diff, model, cu(torch.from_numpy(fx["x_start"].astype(np.float32))), 0, False)
    fx = H.load("sample_ragged_x0")
    meta = H.sample_meta(fx)
    model, diff = dnn_pair(meta, fx)
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    same(diff, model, x, 2, True, noise0=cu(torch.from_numpy(fx["noise_noisy0"])),
         step_noise=cu(torch.from_numpy(fx["noise_noisy_steps"])))  # sampling noise
    cap_a, cap_b = {}, {}
    item = diff.p_sample(model, x, 0, False, capture=cap_a)  # capture
    lat = diff.p_sample(model, x, 0, False, capture=cap_b, latent=True)
    assert diff.last_reverse_route == "item" and torch.equal(lat, item) and len(cap_b["mean"]) == meta["T"]
    model16, _ = dnn_pair(meta, fx, gemm_dtype="bf16")  # bf16 products
    same(diff, model16, x, 0, False)
    fx = H.load("dnncat_sample_tiny_x0")  # DNNCat
    meta = H.onehot_sample_meta(fx)
    I, dims = meta["I"], meta["dims"]
    cat = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], 10)
    cat.load_state_dict(H.state_dict_from(fx))
    cat = cat.to(DEV).eval()
    dd = gdmcf_amd.GaussianDiffusionDiscrete(_mt(meta), "linear-var", meta["scale"], meta["nmin"], meta["nmax"], meta["T"], DEV,
                                             discrete=meta["discrete"], CatOneHot=True)
    same(dd, cat, cu(torch.from_numpy(fx["x_start"].astype(np.float32))), 0, False)


# ---------------------------------------------------------------------------------------------------------------------
# freshness: the cached operands follow the weights
# ---------------------------------------------------------------------------------------------------------------------
def _assert_follows(monkeypatch, model, diff, meta, x, got, before):
    ref = _oracle64(monkeypatch, model, meta, x)
    scale = max(np.abs(ref).max(), 1.0)
    moved = np.abs(ref - before).max()
    assert moved > 100 * 2e-5 * scale, moved  # the step really moved the result: stale operands cannot pass below
    assert np.abs(got.cpu().double().numpy() - ref).max() < 2e-5 * scale
    return ref


def test_latent_operands_follow_an_eager_optimiser_step(monkeypatch):
    I, B = 131, 10
    model, diff, meta = _fresh_dnn(I, [24], [24], 5, seed=4)
    x = _rows(B, I, 6)
    before = _oracle64(monkeypatch, model, meta, x)
    first = diff.p_sample(model, cu(x), 0, False, latent=True)
    assert np.abs(first.cpu().double().numpy() - before).max() < 2e-5 * max(np.abs(before).max(), 1.0)
    ops = model.engine._latent[1]
    assert diff.p_sample(model, cu(x), 0, False, latent=True) is not None and model.engine._latent[1] is ops  # cached
    opt = torch.optim.Adam(model.parameters(), lr=0.02)  # (every weight moves by about lr, whatever the gradient's scale)
    model.train()
    model.drop.p = 0.0
    diff.training_losses(model, cu(x))["loss"].mean().backward()
    opt.step()
    model.eval()
    second = diff.p_sample(model, cu(x), 0, False, latent=True)
    assert diff.last_reverse_route == "latent" and model.engine._latent[1] is not ops
    _assert_follows(monkeypatch, model, diff, meta, x, second, before)


def test_cached_operands_follow_graph_replays(monkeypatch):
    """A replayed training step rewrites the weights without Python: GraphedTrainStep moves the version counters after every replay
    (and in close()), which the latent operands AND the cached transposes of the item-space route (the CSR rows' first-layer gather)
    compare."""
    from gdmcf_amd.graph import GraphedTrainStep
    U, I, B, T = 200, 301, 32, 5
    rng = np.random.default_rng(9)
    dense = (rng.random((U, I)) < 0.05).astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    model, diff, meta = _fresh_dnn(I, [24], [24], T, seed=8, scale=0.1)
    model.train()
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=2e-2, weight_decay=0.0)
    x = torch.from_numpy(dense[:10])
    batches = [torch.from_numpy(np.random.default_rng(500 + k).permutation(U)[:B].astype(np.int64)) for k in range(6)]

    def both():
        model.eval()
        lat = diff.p_sample(model, cu(x), 0, False, latent=True)
        assert diff.last_reverse_route == "latent"
        item = diff.p_sample(model, csr_batch(x.numpy()), 0, False)
        assert diff.last_reverse_route == "item"
        model.train()
        return lat, item

    with GraphedTrainStep(diff, model, opt, dcsr, B, warmup=2) as gstep:
        for b in batches[:3]:
            gstep(b)  # two eager steps, then the capture and its first replay
        assert isinstance(gstep.graph, torch.cuda.CUDAGraph)
        before = _oracle64(monkeypatch, model, meta, x)
        both()  # fills both caches
        for b in batches[3:5]:
            gstep(b)  # replays only
        lat, item = both()
        after = _assert_follows(monkeypatch, model, diff, meta, x, lat, before)
        assert np.abs(item.cpu().double().numpy() - after).max() < 2e-5 * max(np.abs(after).max(), 1.0)
        gstep(batches[5])
    lat, item = both()  # after close()
    final = _assert_follows(monkeypatch, model, diff, meta, x, lat, before)
    assert np.abs(item.cpu().double().numpy() - final).max() < 2e-5 * max(np.abs(final).max(), 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the route is really taken
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 6])
@pytest.mark.parametrize("sparse", [False, True])
def test_latent_loop_makes_two_item_wide_products_whatever_T(monkeypatch, T, sparse):
    I, B = 131, 10
    model, diff, _ = _fresh_dnn(I, [24], [24], T, seed=5)
    x = _rows(B, I, 7)
    rows = csr_batch(x.numpy()) if sparse else cu(x)
    diff.p_sample(model, rows, 0, False, latent=True)  # builds the operands (their own item-wide product, once per weight version)
    calls = []

    def spy(name, shape_of):
        real = getattr(core, name)
        monkeypatch.setattr(core, name, lambda *a: (calls.append((name,) + shape_of(a)), real(*a))[1])

    spy("linear_fwd", lambda a: (a[7], a[8]))            # (N, K)
    spy("linear_bwd_input", lambda a: (a[8], a[9]))
    spy("posterior_fwd", lambda a: (a[12], a[13]))
    spy("gather_fwd", lambda a: (a[3] is not None,))      # (gathers CSR rows,)
    spy("latent_step", lambda a: (a[10], a[11]))
    diff.p_sample(model, rows, 0, False, latent=True)
    assert diff.last_reverse_route == "latent"
    first = [c for c in calls if (c[0] == "linear_fwd" and c[2] == I) or (c[0] == "gather_fwd" and c[1])]
    last = [c for c in calls if c[0] == "posterior_fwd"]
    assert len(first) == 1 and first[0][0] == ("gather_fwd" if sparse else "linear_fwd")
    assert last == [("posterior_fwd", I, 24)]
    assert calls.count(("latent_step", 24, 24)) == T - 1
    assert not [c for c in calls if c[0] == "linear_bwd_input"]  # the operands came from the cache
    assert not [c for c in calls if c[0] == "linear_fwd" and I in c[1:] and c not in first]


# ---------------------------------------------------------------------------------------------------------------------
# driver.evaluate(latent=True)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_evaluate_latent_takes_the_latent_route_on_every_batch(monkeypatch, sparse):
    U, I, bs, topN = 25, 131, 8, [5, 10]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    model, diff, _ = _fresh_dnn(I, [24], [24], 5, seed=2)
    routes = []
    real = diff.p_sample

    def spy(m, b, *a, **kw):
        out = real(m, b, *a, **kw)
        routes.append((b.shape[0], kw.get("latent"), diff.last_reverse_route))
        return out

    monkeypatch.setattr(diff, "p_sample", spy)
    got = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, sparse=sparse, latent=True)
    assert routes == [(8, True, "latent")] * 3 + [(1, True, "latent")]
    dcsr, lists = DeviceCSR(train, DEV), []
    for lo in range(0, U, bs):
        rows = np.arange(lo, min(lo + bs, U))
        ids = torch.from_numpy(rows)
        pred = real(model, dcsr.batch(ids) if sparse else dcsr.rows(ids), 0, False, latent=True)
        indptr, cols = gdmcf_amd.evaluate_utils.csr_rows_to_device(train, rows, DEV)
        lists.append(gdmcf_amd.masked_topk(pred, topN[-1], indptr, cols))
    want = gdmcf_amd.evaluate_utils.computeTopNAccuracy_device(test, torch.cat(lists), topN)
    assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
