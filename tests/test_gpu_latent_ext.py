"""GPU: the latent reverse loop and `recommend` for the EPSILON target and `DNNCat` (`latent="extended"`).
gdmcf_latent_step_ex_f32 against gdmcf_latent_step_f32 (bit for bit without its optional parts) and against a float64 evaluation
with them; gdmcf_latent_acc_f32; the four loops against the reference fixtures; the embedding backbones, a deep DNN and DNNCat
against float64 oracles; recommend's lists; the launches the routes really make; freshness after an optimiser step."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn as nn

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from gdmcf_amd.data_utils import DeviceCSR
from gdmcf_amd.recommend import recommend
from oracle import gdmcf_oracle as O
from tests import helpers as H
from tests.test_gpu_latent import _discrete, _oracle_discrete64, _rows, csr_batch, cu, dnn_pair
from tests.test_gpu_recommend import _check_lists, _draws

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24

# ---------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
# B not a multiple of 16, N not a multiple of 64, K below 16, K with unequal chunk counts per wave, the partial last chunk; the last
# entry: odd leading dimensions and pointers one float off a 16-byte boundary (the scalar paths)
SHAPES = [(1, 1, 1, 0), (7, 24, 50, 0), (37, 100, 83, 0), (129, 200, 257, 0), (400, 1000, 1000, 0), (37, 100, 97, 1)]
_PROBLEMS = {}


def _ld(n, odd):
    return n + 1 + (n % 2) if odd else (n + 3) // 4 * 4 + 8


def _inside_nans(data, odd):
    """`data` [rows, n] inside a NaN-filled device buffer: padded rows, and with `odd` a first element one float behind a
    16-byte boundary."""
    rows, n = data.shape
    ld = _ld(n, odd)
    flat = torch.full((rows * ld + 8,), float("nan"), device=DEV)
    t = flat[4 + odd: 4 + odd + rows * ld].view(rows, ld)
    t[:, :n] = data.to(DEV)
    return t


def _vec(data, odd):
    flat = torch.full((data.numel() + 8,), float("nan"), device=DEV)
    t = flat[4 + odd: 4 + odd + data.numel()]
    t.copy_(data)
    return t


def _problem(B, N, K, odd):
    """Operands (device, inside NaN-filled buffers) and the float64 reference with its bounds; made once, never modified."""
    key = (B, N, K, odd)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(5 * B + 3 * N + 17 * K + odd)
    rnd = lambda *s: torch.randn(*s, generator=g)
    A, M = torch.tanh(rnd(B, K)), rnd(N, K) * (2.0 / K ** 0.5)
    v, e, pc, r, qc = rnd(N) * 0.3, rnd(N) * 0.3, rnd(B, N), rnd(B, N) * 0.5, rnd(B, K)
    c1, c2 = torch.rand(B, generator=g) * 0.9 + 0.1, torch.rand(B, generator=g) * 0.9
    qa, qb = torch.rand(B, generator=g) + 0.5, rnd(B)
    qa[::3] = 0.0  # rows that must not read q_cur
    d = lambda t: t.double()
    s, sabs = d(A) @ d(M).t(), d(A).abs() @ d(M).abs().t()
    pn = d(c1)[:, None] * (s + d(v)) + d(c2)[:, None] * d(pc)
    bp = (K + 6) * U24 * (d(c1)[:, None] * (sabs + d(v).abs()) + d(c2)[:, None] * d(pc).abs())  # tests/test_gpu_latent._reference
    h = torch.tanh((pn + d(r)) + d(e))
    bh = bp + 2 * U24 * (pn.abs() + d(r).abs() + d(e).abs()) + 4 * U24
    qn = d(qa)[:, None] * d(qc) + d(qb)[:, None] * d(A)
    bq = 2 * U24 * ((d(qa)[:, None] * d(qc)).abs() + (d(qb)[:, None] * d(A)).abs())
    P = dict(A=_inside_nans(A, odd), M=_inside_nans(M, odd), pc=_inside_nans(pc, odd), r=_inside_nans(r, odd), qc=_inside_nans(qc, odd),
             v=_vec(v, odd), e=_vec(e, odd), c1=_vec(c1, 0), c2=_vec(c2, 0), qa=_vec(qa, 0), qb=_vec(qb, 0),
             pn=pn, bp=bp, h=h, bh=bh, qn=qn, bq=bq)
    _PROBLEMS[key] = P
    return P


def _out(rows, n, odd):
    return _inside_nans(torch.full((rows, n), 7.0), odd)


def _ex(P, B, N, K, odd, use_r=True, use_q=True, q_inplace=False, out=None):
    """One gdmcf_latent_step_ex_f32 launch with v, e and tanh; returns (p_next, h_next, q_next)."""
    lib = _lib.load()
    pn, h = out if out is not None else (_out(B, N, odd), _out(B, N, odd))
    qcur = P["qc"].clone() if q_inplace else P["qc"]
    if q_inplace and odd:  # (clone() packs the rows: put them back on the odd leading dimension)
        qcur = _inside_nans(P["qc"][:, :K].cpu(), odd)
    qn = (qcur if q_inplace else _out(B, K, odd)) if use_q else None
    p2 = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
    _lib.check(lib.gdmcf_latent_step_ex_f32(
        *p2(P["A"]), *p2(P["M"]), P["v"].data_ptr(), *p2(P["pc"]), P["c1"].data_ptr(), P["c2"].data_ptr(),
        *(p2(P["r"]) if use_r else (None, 0)), P["e"].data_ptr(), 1, B, N, K, *p2(pn), *p2(h),
        *(p2(qcur) if use_q else (None, 0)), P["qa"].data_ptr() if use_q else None, P["qb"].data_ptr() if use_q else None, *p2(qn),
        None, 0, _lib.stream_ptr()))
    return pn, h, qn


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("B,N,K,odd", SHAPES)
def test_ex_entry_without_its_parts_equals_the_old_entry_bit_for_bit(B, N, K, odd):
    P = _problem(B, N, K, odd)
    lib = _lib.load()
    pn, h = _out(B, N, odd), _out(B, N, odd)
    _lib.check(lib.gdmcf_latent_step_f32(
        P["A"].data_ptr(), P["A"].stride(0), P["M"].data_ptr(), P["M"].stride(0), P["v"].data_ptr(), P["pc"].data_ptr(),
        P["pc"].stride(0), P["c1"].data_ptr(), P["c2"].data_ptr(), P["e"].data_ptr(), 1, B, N, K, pn.data_ptr(), pn.stride(0),
        h.data_ptr(), h.stride(0), None, 0, _lib.stream_ptr()))
    pn2, h2, _ = _ex(P, B, N, K, odd, use_r=False, use_q=False)
    assert bool(torch.isfinite(pn[:, :N]).all()) and bool(torch.isfinite(h[:, :N]).all())
    assert _same_bits(pn2, pn) and _same_bits(h2, h)  # (padding included: both keep their NaNs)


@pytest.mark.parametrize("B,N,K,odd", SHAPES)
def test_ex_entry_with_row_addend_and_accumulator_matches_float64(B, N, K, odd):
    P = _problem(B, N, K, odd)
    pn, h, qn = _ex(P, B, N, K, odd)
    err_p = (pn[:, :N].cpu().double() - P["pn"]).abs()
    err_h = (h[:, :N].cpu().double() - P["h"]).abs()
    err_q = (qn[:, :K].cpu().double() - P["qn"]).abs()
    for name, err, bound in (("p_next", err_p, P["bp"]), ("h_next", err_h, P["bh"]), ("q_next", err_q, P["bq"])):
        print(f"B={B} N={N} K={K} odd={odd} {name}: max err {float(err.max()):.3e}, largest err/bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err_p <= P["bp"]).all()) and bool((err_h <= P["bh"]).all()) and bool((err_q <= P["bq"]).all())
    # padding columns keep their NaNs; nothing was written behind column N / K
    assert bool(torch.isnan(h[:, N:]).all()) and bool(torch.isnan(qn[:, K:]).all()) and bool(torch.isnan(pn[:, N:]).all())
    # determinism, and the parts do not disturb p_next
    pn2, h2, qn2 = _ex(P, B, N, K, odd)
    assert _same_bits(pn2, pn) and _same_bits(h2, h) and _same_bits(qn2, qn)
    assert _same_bits(_ex(P, B, N, K, odd, use_r=False, use_q=False)[0], pn)
    # in place
    _, _, qi = _ex(P, B, N, K, odd, q_inplace=True)
    assert _same_bits(qi[:, :K], qn[:, :K]) and bool(torch.isnan(qi[:, K:]).all())
    # the stand-alone launch: the same bits
    lib = _lib.load()
    qs = _out(B, K, odd)
    _lib.check(lib.gdmcf_latent_acc_f32(P["qc"].data_ptr(), P["qc"].stride(0), P["qa"].data_ptr(), P["A"].data_ptr(), P["A"].stride(0),
                                        P["qb"].data_ptr(), B, K, qs.data_ptr(), qs.stride(0), _lib.stream_ptr()))
    assert _same_bits(qs, qn)


@pytest.mark.parametrize("B,N,K,odd", [(37, 100, 83, 0), (37, 100, 97, 1)])
def test_rows_with_qa_zero_do_not_read_q_cur(B, N, K, odd):
    P = _problem(B, N, K, odd)
    poisoned = dict(P, qc=_inside_nans(torch.full((B, K), float("nan")), odd), qa=torch.zeros(B, device=DEV))
    _, _, qn = _ex(poisoned, B, N, K, odd)
    assert bool(torch.isfinite(qn[:, :K]).all())
    want = (P["qb"][:B, None] * P["A"][:, :K])
    assert torch.equal(qn[:, :K], want)


def test_ex_kernel_is_capture_safe():
    """One linear chain, no parallel branches: the captured launch replays the eager bits."""
    B, N, K = 37, 100, 83
    P = _problem(B, N, K, 0)
    want = _ex(P, B, N, K, 0)
    outs = (_out(B, N, 0), _out(B, N, 0))
    lib = _lib.load()
    qn = _out(B, K, 0)
    p2 = lambda t: (t.data_ptr(), t.stride(0))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.check(lib.gdmcf_latent_step_ex_f32(
            *p2(P["A"]), *p2(P["M"]), P["v"].data_ptr(), *p2(P["pc"]), P["c1"].data_ptr(), P["c2"].data_ptr(), *p2(P["r"]),
            P["e"].data_ptr(), 1, B, N, K, *p2(outs[0]), *p2(outs[1]), *p2(P["qc"]), P["qa"].data_ptr(), P["qb"].data_ptr(), *p2(qn),
            None, 0, _lib.stream_ptr()))
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(outs[0], want[0]) and _same_bits(outs[1], want[1]) and _same_bits(qn, want[2])


# ---------------------------------------------------------------------------------------------------------------------
# the loops against the reference fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _topk_sets(pred, x, k):
    """Sets of the k largest unmasked items per row (float64 on the host)."""
    p = np.where(x != 0, -np.inf, np.asarray(pred, dtype=np.float64))
    return [set(np.argsort(-p[b], kind="stable")[:k].tolist()) for b in range(p.shape[0])]


def _against_fixture(got, ref, x, what):
    ref = np.asarray(ref, dtype=np.float64)
    tol = 2e-5 * max(np.abs(ref).max(), 1.0)
    dev = np.abs(got.cpu().double().numpy() - ref).max()
    print(f"{what}: deviation {dev:.3e}, tolerance {tol:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape and dev < tol
    for k in (1, 10, 20):
        assert _topk_sets(got.cpu().numpy(), x, k) == _topk_sets(ref, x, k), (what, k)


def _fixture_pair(name):
    fx = H.load(name)
    if name.startswith("sample_"):
        meta = H.sample_meta(fx)
        model, diff = dnn_pair(meta, fx)
        return fx, meta, model, diff
    meta = H.onehot_sample_meta(fx)
    I, dims = meta["I"], meta["dims"]
    cls = gdmcf_amd.DNNCat if name.startswith("dnncat") else gdmcf_amd.DNNOneHot
    model = cls([I] + dims, dims[::-1] + [I], 10)
    model.load_state_dict(H.state_dict_from(fx))
    return fx, meta, model.to(DEV).eval(), _discrete(meta)


FIXTURES = ["sample_ragged_eps", "onehot_sample_ragged_eps", "dnncat_sample_tiny_x0", "dnncat_sample_ragged_eps"]


@pytest.mark.parametrize("name", FIXTURES)
def test_extended_latent_loops_match_the_reference_fixtures(name):
    fx, meta, model, diff = _fixture_pair(name)
    x64 = fx["x_start"]
    x = cu(torch.from_numpy(x64.astype(np.float32)))
    for rows in (x, csr_batch(x64)):
        p0 = diff.p_sample(model, rows, 0, False, latent="extended")
        assert diff.last_reverse_route == "latent"
        _against_fixture(p0, fx["pred_steps0"], x64, f"{name} steps=0 {type(rows).__name__}")
    inj = dict(noise0=cu(torch.from_numpy(fx["noise_stepsT"])))
    if "sampled_stepsT" in fx:
        inj["sampled0"] = cu(torch.from_numpy(fx["sampled_stepsT"]))
    pT = diff.p_sample(model, x, meta["T"], False, latent="extended", **inj)
    assert diff.last_reverse_route == "latent"
    _against_fixture(pT, fx["pred_stepsT"], x64, f"{name} steps=T")
    # latent=True keeps its answer for these configurations: the item-space route, to the bit
    item = diff.p_sample(model, x, 0, False)
    assert diff.last_reverse_route == "item"
    assert torch.equal(diff.p_sample(model, x, 0, False, latent=True), item) and diff.last_reverse_route == "item"


# ---------------------------------------------------------------------------------------------------------------------
# float64 oracles
# ---------------------------------------------------------------------------------------------------------------------
class _CatOracle(nn.Module):
    """DNNCat for the oracle's GaussianDiffusionDiscrete: cat_layer mixes x_t with the item's one-hot pair, then the oracle DNN's
    layers.  Parameter names are gdmcf_amd.DNNCat's."""

    def __init__(self, in_dims, out_dims, emb_size):
        super().__init__()
        self.time_emb_dim = emb_size
        self.emb_layer = nn.Linear(emb_size, emb_size)
        self.cat_layer = nn.Linear(3, 1)
        ind = [in_dims[0] + emb_size] + list(in_dims[1:])
        self.in_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(ind[:-1], ind[1:])])
        self.out_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(out_dims[:-1], out_dims[1:])])

    def forward(self, x, timesteps, x_U):
        emb = self.emb_layer(O.timestep_embedding(timesteps, self.time_emb_dim))
        z = self.cat_layer(torch.cat([x.unsqueeze(-1), x_U.reshape(x.shape[0], -1, 2).to(x.dtype)], dim=2)).squeeze(-1)
        h = torch.cat([z, emb], dim=-1)
        for layer in self.in_layers:
            h = torch.tanh(layer(h))
        for i, layer in enumerate(self.out_layers):
            h = layer(h)
            if i != len(self.out_layers) - 1:
                h = torch.tanh(h)
        return h


def _mt(name, mod):
    return {"x0": mod.ModelMeanType.START_X, "eps": mod.ModelMeanType.EPSILON}[name]


def _cat_case(mean_type, dims=(24,), seed=31, T=5):
    """(model, diffusion, oracle model, oracle diffusion) of a fresh DNNCat with a cat layer well away from the identity."""
    torch.manual_seed(seed)
    I, dims = 131, list(dims)
    model = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], 10)
    with torch.no_grad():
        model.cat_layer.weight.copy_(torch.tensor([[0.7, -0.3, 0.5]]))
        model.cat_layer.bias.fill_(0.11)
    om = _CatOracle([I] + dims, dims[::-1] + [I], 10)
    om.load_state_dict(model.state_dict())
    meta = dict(mean_type=mean_type, scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99)
    od = O.GaussianDiffusionDiscrete(_mt(mean_type, O), "linear-var", 0.01, 0.001, 0.01, T, discrete=0.99, CatOneHot=True)
    return model.to(DEV).eval(), _discrete(meta), om, od


def _within(got, ref, what):
    ref = np.asarray(ref, dtype=np.float64)
    tol = 2e-5 * max(np.abs(ref).max(), 1.0)
    dev = np.abs(got.cpu().double().numpy() - ref).max()
    print(f"{what}: deviation {dev:.3e}, tolerance {tol:.3e}")
    assert got.dtype == torch.float32 and got.shape == ref.shape and dev < tol


def _three_inputs(monkeypatch, model, diff, x, ref_of, index=None):
    """steps = 0 from dense and from CSR rows, steps = T from dense rows with injected draws."""
    B, I = x.shape
    noise0, sampled0 = _draws(B, I)
    onehot = isinstance(diff, gdmcf_amd.GaussianDiffusionDiscrete) and diff.CatOneHot
    kw = dict(index=index) if index is not None else {}
    for steps, rows in ((0, cu(x)), (0, csr_batch(x.numpy())), (diff.steps, cu(x))):
        inj = {} if steps == 0 else (dict(noise0=noise0, sampled0=sampled0) if onehot else dict(noise0=noise0))
        got = diff.p_sample(model, rows, steps, False, latent="extended", **kw, **{k: cu(v) for k, v in inj.items()})
        assert diff.last_reverse_route == "latent"
        _within(got, ref_of(steps, inj), f"{type(model).__name__} steps={steps} {type(rows).__name__}")


@pytest.mark.parametrize("backbone,dims", [("emb", (32, 24)), ("gcn", (24,))])
def test_embedding_backbones_under_eps_match_float64_oracle(monkeypatch, backbone, dims):
    """tests/test_gpu_latent.test_embedding_backbones_latent_match_float64_oracle under the EPSILON target."""
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
    od = O.GaussianDiffusionDiscrete(O.ModelMeanType.EPSILON, "linear-var", 0.01, 0.001, 0.01, T, CatOneHot=True)
    od.indexIn = True
    diff = _discrete(dict(mean_type="eps", scale=0.01, nmin=0.001, nmax=0.01, T=T, discrete=0.99), index_in=True)
    x = _rows(B, I, 21)
    index = torch.randperm(U, generator=torch.Generator().manual_seed(4))[:B]
    _three_inputs(monkeypatch, gm, diff, x, lambda steps, inj: _oracle_discrete64(monkeypatch, om, od, x, steps, index=index, **inj),
                  index=index)


def _dnn_eps(dims_in, dims_out, seed, T=5, I=131):
    torch.manual_seed(seed)
    model = gdmcf_amd.DNN([I] + dims_in, dims_out + [I], 10, time_type="cat").to(DEV).eval()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.EPSILON, "linear-var", 0.01, 0.001, 0.01, T, DEV).to(DEV)
    om = O.DNN([I] + dims_in, dims_out + [I], 10)
    od = O.GaussianDiffusion(O.ModelMeanType.EPSILON, "linear-var", 0.01, 0.001, 0.01, T)
    return model, diff, om, od


def _dnn_oracle64(monkeypatch, model, om, od, x, steps, noise0=None):
    real = O.timestep_embedding
    monkeypatch.setattr(O, "timestep_embedding", lambda t, d, *a: real(t, d, *a).double())
    om.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    om = om.double().eval()
    with torch.no_grad():
        return od.p_sample(om, x.cpu().double(), steps, False, noise0=None if noise0 is None else noise0.double()).numpy()


def test_deep_dnn_under_eps_matches_float64_oracle(monkeypatch):
    """Two hidden layers on either side (K != h): small layers run between the step kernel's h_next and the accumulated A."""
    model, diff, om, od = _dnn_eps([24, 40], [40, 24], seed=3)
    x = _rows(10, 131, 1)
    _three_inputs(monkeypatch, model, diff, x, lambda steps, inj: _dnn_oracle64(monkeypatch, model, om, od, x, steps, **inj))


def _cat_oracle64(monkeypatch, model, om, od, x, steps, noise0=None, sampled0=None):
    om.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    return _oracle_discrete64(monkeypatch, om, od, x, steps, noise0=noise0, sampled0=sampled0)


@pytest.mark.parametrize("mean_type,dims", [("x0", (24,)), ("eps", (24, 40))])
def test_dnncat_matches_float64_oracle(monkeypatch, mean_type, dims):
    model, diff, om, od = _cat_case(mean_type, dims)
    x = _rows(10, 131, 23)
    _three_inputs(monkeypatch, model, diff, x, lambda steps, inj: _cat_oracle64(monkeypatch, model, om, od, x, steps, **inj))


# ---------------------------------------------------------------------------------------------------------------------
# recommend(latent="extended")
# ---------------------------------------------------------------------------------------------------------------------
def _rec_case(name, monkeypatch):
    """(model, diffusion, x, ref_of(steps, noise0, sampled0))"""
    x = _rows(10, 131, 29)
    if name == "dnn_eps":
        model, diff, om, od = _dnn_eps([24], [24], seed=6)
        return model, diff, x, lambda steps, nz, sm: _dnn_oracle64(monkeypatch, model, om, od, x, steps, nz)
    if name == "onehot_eps":
        fx = H.load("onehot_sample_ragged_eps")
        meta = H.onehot_sample_meta(fx)
        I, dims = meta["I"], meta["dims"]
        model = gdmcf_amd.DNNOneHot([I] + dims, dims[::-1] + [I], 10)
        model.load_state_dict(H.state_dict_from(fx))
        om, od = H.oracle_onehot_pair(meta, fx)
        x = torch.from_numpy(fx["x_start"].astype(np.float32))
        return model.to(DEV).eval(), _discrete(meta), x, \
            lambda steps, nz, sm: _oracle_discrete64(monkeypatch, om, od, x, steps, noise0=nz, sampled0=sm)
    model, diff, om, od = _cat_case("x0" if name == "cat_x0" else "eps")
    return model, diff, x, lambda steps, nz, sm: _cat_oracle64(monkeypatch, model, om, od, x, steps, nz, sm)


@pytest.mark.parametrize("name", ["dnn_eps", "onehot_eps", "cat_x0", "cat_eps"])
def test_recommend_extended_matches_the_float64_oracle(monkeypatch, name):
    model, diff, x, ref_of = _rec_case(name, monkeypatch)
    B, I = x.shape
    ids = torch.arange(B)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    noise0, sampled0 = _draws(B, I)
    onehot = isinstance(diff, gdmcf_amd.GaussianDiffusionDiscrete)
    eps = diff.mean_type == ModelMeanType.EPSILON
    no_mask = "latent" if eps else "latent-csr"  # eps ranks without G x_T only where the rows themselves are masked
    for steps, mask, route in ((0, "rows", "latent-csr"), (0, None, no_mask), (diff.steps, "rows", "latent")):
        inj = {} if steps == 0 else (dict(noise0=noise0, sampled0=sampled0) if onehot else dict(noise0=noise0))
        ref = ref_of(steps, inj.get("noise0"), inj.get("sampled0"))
        masked = (x.numpy() != 0) if mask == "rows" else np.zeros(x.shape, dtype=bool)
        for k in (1, 20):
            val, idx = recommend(diff, model, dcsr, ids, k, mask=mask, sampling_steps=steps, return_values=True, latent="extended", **inj)
            assert diff.last_recommend_route == route and diff.last_reverse_route == "latent"
            _check_lists(val, idx, ref, masked, k, f"{name} steps={steps} mask={mask} k={k}")
        # latent=True (the default) is unchanged: the item-space route and evaluate's bits
        val, idx = recommend(diff, model, dcsr, ids, 20, mask=mask, sampling_steps=steps, return_values=True, **inj)
        assert diff.last_recommend_route == "item"
        pred = diff.p_sample(model, dcsr.rows(ids), steps, False, **{k_: cu(v) for k_, v in inj.items()})
        his = gdmcf_amd.evaluate_utils.csr_rows_to_device(sp.csr_matrix(x.numpy()), np.arange(B), DEV) if mask == "rows" else ()
        want = gdmcf_amd.evaluate_utils.masked_topk(pred, 20, *his, return_values=True)
        assert torch.equal(idx, want[1]) and torch.equal(val, want[0])


# ---------------------------------------------------------------------------------------------------------------------
# the launches the routes really make
# ---------------------------------------------------------------------------------------------------------------------
def _count_calls(monkeypatch, lib, names):
    """Counts C-ABI calls by entry point: (name, args) per call."""
    calls = []
    for name in names:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, (lambda nm, fn: lambda *a: (calls.append((nm, a)), fn(*a))[1])(name, real), raising=False)
    return calls


ENTRIES = ["gdmcf_cat_prep_input_f32", "gdmcf_cat_prep_input_csr_f32", "gdmcf_onehot_noise_f32", "gdmcf_linear_posterior_fwd_f32",
           "gdmcf_linear_fwd_f32", "gdmcf_linear_fwd_wt_f32", "gdmcf_latent_step_f32", "gdmcf_latent_step_ex_f32",
           "gdmcf_latent_acc_f32", "gdmcf_dnn_prep_input_f32", "gdmcf_dnn_prep_input_csr_f32"]


def _item_wide(calls, I):
    """Products with N = I or K = I (gdmcf_linear_fwd*_f32: ..., act, M, N, K at positions 6, 7, 8)."""
    return [c for c in calls if c[0].startswith("gdmcf_linear_fwd") and I in (c[1][7], c[1][8])] + \
        [c for c in calls if c[0] == "gdmcf_linear_posterior_fwd_f32"]


@pytest.mark.parametrize("T", [3, 6])
@pytest.mark.parametrize("case", ["cat_x0", "dnn_eps"])
def test_extended_latent_csr_route_launches(monkeypatch, T, case):
    I, U = 131, 10
    x = _rows(U, I, 7)
    if case == "cat_x0":
        model, diff, _, _ = _cat_case("x0", T=T)
    else:
        model, diff, _, _ = _dnn_eps([24], [24], seed=5, T=T)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    ids = torch.arange(U)
    recommend(diff, model, dcsr, ids, 5, latent="extended")  # builds the cached operands
    calls = _count_calls(monkeypatch, model.engine.lib, ENTRIES)
    recommend(diff, model, dcsr, ids, 5, latent="extended")
    assert diff.last_recommend_route == "latent-csr"
    names = [c[0] for c in calls]
    for absent in ("gdmcf_cat_prep_input_f32", "gdmcf_cat_prep_input_csr_f32", "gdmcf_onehot_noise_f32", "gdmcf_dnn_prep_input_f32",
                   "gdmcf_dnn_prep_input_csr_f32", "gdmcf_linear_posterior_fwd_f32"):
        assert absent not in names, absent
    wide = _item_wide(calls, I)
    assert len(wide) == 1 and wide[0][1][7] == I  # exactly one product with N = I
    steps = [c for c in calls if c[0] in ("gdmcf_latent_step_f32", "gdmcf_latent_step_ex_f32")]
    assert len(steps) == T - 1
    if case == "dnn_eps":
        # T accumulations: one fused into every step (its q_next argument, position 24, is given), one launch for the last step
        fused = [c for c in steps if c[0] == "gdmcf_latent_step_ex_f32" and c[1][24] is not None]
        assert len(fused) == T - 1 and names.count("gdmcf_latent_acc_f32") == 1


@pytest.mark.parametrize("T", [3, 6])
def test_dense_dnncat_makes_at_most_three_item_wide_products(monkeypatch, T):
    I, B = 131, 10
    model, diff, _, _ = _cat_case("eps", T=T)
    x = cu(_rows(B, I, 7))
    diff.p_sample(model, x, 0, False, latent="extended")
    calls = _count_calls(monkeypatch, model.engine.lib, ENTRIES)
    diff.p_sample(model, x, 0, False, latent="extended")
    assert diff.last_reverse_route == "latent"
    assert len(_item_wide(calls, I)) <= 3
    assert [c[0] for c in calls].count("gdmcf_cat_prep_input_f32") == 1


# ---------------------------------------------------------------------------------------------------------------------
# freshness
# ---------------------------------------------------------------------------------------------------------------------
def test_extended_lists_follow_an_eager_optimiser_step(monkeypatch):
    """One eager optimiser step moves cat_layer and W1: the cached operands (M, v, S), the time table with (w1 + c) S and the
    step table c1 . w0 must all follow."""
    model, diff, om, od = _cat_case("x0")
    x = _rows(10, 131, 6)
    B = x.shape[0]
    ids = torch.arange(B)
    dcsr = DeviceCSR(sp.csr_matrix(x.numpy().astype(np.float64)), DEV)
    masked = x.numpy() != 0
    before = _cat_oracle64(monkeypatch, model, om, od, x, 0)
    val, idx = recommend(diff, model, dcsr, ids, 20, return_values=True, latent="extended")
    assert diff.last_recommend_route == "latent-csr"
    _check_lists(val, idx, before, masked, 20, "before the step")
    opt = torch.optim.Adam(model.parameters(), lr=0.02)  # (every parameter moves by about lr)
    w1_before, cat_before = model.in_layers[0].weight.detach().clone(), model.cat_layer.weight.detach().clone()
    model.train()
    model.drop.p = 0.0
    diff.training_losses(model, cu(x))["loss"].mean().backward()
    opt.step()
    model.eval()
    assert not torch.equal(model.in_layers[0].weight, w1_before) and not torch.equal(model.cat_layer.weight, cat_before)
    after = _cat_oracle64(monkeypatch, model, om, od, x, 0)
    tol = 2e-5 * max(np.abs(after).max(), 1.0)
    assert np.abs(after - before).max() > 100 * tol  # the step really moved the result: stale operands cannot pass below
    for mask in ("rows", None):
        val, idx = recommend(diff, model, dcsr, ids, 20, mask=mask, return_values=True, latent="extended")
        assert diff.last_recommend_route == "latent-csr"
        _check_lists(val, idx, after, masked if mask == "rows" else np.zeros_like(masked), 20, f"after the step, mask={mask}")


# ---------------------------------------------------------------------------------------------------------------------
# driver.evaluate(latent="extended")
# ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_passes_the_extended_spelling_through(monkeypatch):
    from gdmcf_amd import driver
    U, I, bs, topN = 25, 131, 8, [5, 10]
    rng = np.random.default_rng(3)
    train = sp.csr_matrix((rng.random((U, I)) < 0.12).astype(np.float64))
    test = sp.csr_matrix((rng.random((U, I)) < 0.05).astype(np.float64))
    model, diff, _, _ = _dnn_eps([24], [24], seed=2)
    routes = []
    real = diff.p_sample

    def spy(m, b, *a, **kw):
        out = real(m, b, *a, **kw)
        routes.append((b.shape[0], kw.get("latent"), diff.last_reverse_route))
        return out

    monkeypatch.setattr(diff, "p_sample", spy)
    ext = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, sparse=True, latent="extended")
    assert routes == [(8, "extended", "latent")] * 3 + [(1, "extended", "latent")]
    del routes[:]
    item = driver.evaluate(diff, model, train, test, train, topN, 0, False, bs, DEV, sparse=True, latent=True)
    assert routes == [(8, True, "item")] * 3 + [(1, True, "item")]
    # the same users ranked by two routes that agree within float32 rounding: the metrics agree closely
    assert np.allclose(np.asarray(ext, dtype=np.float64), np.asarray(item, dtype=np.float64), atol=0.02)
    dcsr = DeviceCSR(train, DEV)
    driver.evaluate(diff, model, dcsr, test, dcsr, topN, 0, False, bs, DEV, latent="extended", recommend=True)
    assert diff.last_recommend_route == "latent-csr"  # the rows themselves are the mask
    driver.evaluate(diff, model, dcsr, test, dcsr, topN, 0, False, bs, DEV, latent=True, recommend=True)
    assert diff.last_recommend_route == "item"
