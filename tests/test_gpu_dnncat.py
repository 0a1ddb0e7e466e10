"""GPU (-m gpu): the DNNCat backbone -- GaussianDiffusionDiscrete(CatOneHot=True) driving a DNNCat denoiser -- through the C
ABI against the committed outputs of the real reference (tests/golden/dnncat_*.npz, tools/gen_golden_dnncat.py), and the two
kernels of csrc/cat.hip on their own against float32 / float64 torch evaluations on the same GPU."""
import numpy as np
import pytest
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAIN_CASES = ["tiny_x0", "ragged_eps_wd", "deep_x0", "wide_x0"]
SAMPLE_CASES = ["tiny_x0", "ragged_eps"]
SHAPES = {"ragged": (12, 131), "wide": (3, 4100)}  # I % 4 != 0 (float4 tail, odd xU rows); past the 4096-column workgroup
E = 10


def cu(t):
    return t.to(DEV)


def load_train(case):
    fx = H.load("dnncat_train_" + case)
    try:
        fx.update(H.load("dnncat_train_" + case + "_final"))  # (wide_x0 keeps pN / m / v in a second file)
    except FileNotFoundError:
        pass
    return fx


def gpu_pair(meta, fx):
    I, dims = meta["I"], meta["dims"]
    m = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], meta.get("emb", 10))
    m.load_state_dict(H.state_dict_from(fx))
    mt = {"x0": ModelMeanType.START_X, "eps": ModelMeanType.EPSILON}[meta["mean_type"]]
    d = gdmcf_amd.GaussianDiffusionDiscrete(mt, meta.get("schedule", "linear-var"), meta["scale"], meta["nmin"],
                                            meta["nmax"], meta["T"], DEV, discrete=meta["discrete"], CatOneHot=True)
    return m.to(DEV), d


def step_inputs(fx, s):
    p = f"s{s}."
    d = H.step_inputs(fx, s)
    d.update(ts_U=torch.from_numpy(fx[p + "ts_U"]), sampled=torch.from_numpy(fx[p + "sampled"].astype(np.int64)))
    return d


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_dnncat_train_steps_match_reference(case):
    """zero_grad -> training_losses -> mean -> backward -> AdamW.step with the reference's randomness injected (both timestep
    draws, the sampled classes, noise, the dropout keep-mask); tolerances of test_onehot_train_steps_match_reference.  The two
    cat_layer gradients are sums of B x I terms of mixed sign: they are held against the float64 run of the reference
    (g0_f64.*), within max(2e-4, twice the reference's own float32-to-float64 error).  The stored reference errors are
    2.3e-7 / 7.8e-8 (tiny_x0), 3.6e-8 / 2.3e-7 (ragged_eps_wd), 2.2e-7 / 1.4e-7 (deep_x0), 1.6e-7 / 2.4e-8 (wide_x0) for
    weight / bias: no case needs the second term."""
    fx = load_train(case)
    meta = H.onehot_train_meta(fx)
    model, diff = gpu_pair(meta, fx)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    model.train()
    for s in range(meta["n_steps"]):
        inp = step_inputs(fx, s)
        xU, _ = model.engine.onehot_rows(cu(inp["x"]), None, cu(inp["sampled"]), meta["discrete"])
        np.testing.assert_array_equal(xU.cpu().numpy().reshape(meta["B"], meta["I"], 2).astype(np.uint8), fx[f"s{s}.x_tU"])
        opt.zero_grad()
        terms = diff.training_losses(model, cu(inp["x"]), True, ts=cu(inp["ts"]), pt=cu(inp["pt"]), noise=cu(inp["noise"]),
                                     drop_mask=cu(inp["drop_mask"]), ts_U=cu(inp["ts_U"]), sampled=cu(inp["sampled"]))
        assert terms["loss"].dtype == torch.float64 and terms["loss"].shape == (meta["B"],)
        loss = terms["loss"].mean()
        loss.backward()
        bufs = model.engine.buffers(meta["B"], torch.device(DEV))
        np.testing.assert_allclose(bufs.xt[:, :meta["I"]].cpu().numpy(), fx[f"s{s}.x_t"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(terms["loss"].detach().cpu().numpy(), fx[f"s{s}.loss_vec"], rtol=1e-4, atol=0)
        assert abs(float(loss.detach()) - float(fx[f"s{s}.loss"])) <= 1e-4 * abs(float(fx[f"s{s}.loss"]))
        if s == 0:
            for k, v in model.named_parameters():
                got = v.grad.cpu().numpy()
                if k.startswith("cat_layer."):
                    ref_err = H.relerr(fx["g0." + k], fx["g0_f64." + k])
                    err = H.relerr(got, fx["g0_f64." + k])
                    print(f"{case} {k}: error to float64 {err:.3g} (reference's own {ref_err:.3g})")
                    assert err <= max(2e-4, 2 * ref_err), (k, err, ref_err)
                else:
                    assert H.relerr(got, fx["g0." + k]) < 2e-4, k
        opt.step()
        np.testing.assert_array_equal(diff.Lt_count.cpu().numpy(), fx[f"s{s}.Lt_count"])
        np.testing.assert_allclose(diff.Lt_history.cpu().numpy(), fx[f"s{s}.Lt_history"], rtol=1e-4, atol=0)
    for k, v in model.named_parameters():
        d = np.abs(v.detach().cpu().numpy() - fx["pN." + k]).max()
        assert d < 0.02 * meta["lr"] * meta["n_steps"], (k, d)
        assert H.relerr(opt.state[v]["exp_avg"].cpu().numpy(), fx["m." + k]) < 2e-4, k
        assert H.relerr(opt.state[v]["exp_avg_sq"].cpu().numpy(), fx["v." + k]) < 4e-4, k


# ---- the builder alone --------------------------------------------------------------------------------------------------
class _Case:
    """Random operands of one shape, made once per shape (module cache) and never written."""

    def __init__(self, B, I, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.I = B, I
        self.x0 = cu((torch.rand(B, I, generator=g) < 0.1).float())
        s = (torch.rand(B, I, generator=g) < 0.5)
        xu = torch.zeros(B, I, 2)
        xu[..., 0] = (s & (torch.rand(B, I, generator=g) < 0.7)).float()
        xu[..., 1] = (~s & (torch.rand(B, I, generator=g) < 0.7)).float()
        self.xU = cu(xu.reshape(B, 2 * I).contiguous())
        self.noise = cu(torch.randn(B, I, generator=g))
        self.keep = cu((torch.rand(B, I, generator=g) < 0.5).to(torch.uint8))
        self.ts = cu(torch.randint(0, 5, (B,), generator=g))
        self.ca = cu(torch.rand(5, generator=g) * 0.5 + 0.5)
        self.cb = cu(torch.rand(5, generator=g) * 0.5)
        self.w = cu(torch.randn(1, 3, generator=g))
        self.c = cu(torch.randn(1, generator=g))
        self.emb_w = cu(torch.randn(E, E, generator=g) * 0.3)
        self.emb_b = cu(torch.randn(E, generator=g) * 0.01)
        self.dxin = cu(torch.randn(B, I, generator=g))
        self.ld = (I + E + 63) // 64 * 64
        self.ldi = (I + 63) // 64 * 64


_CASES = {}


def case_of(name):
    if name not in _CASES:
        B, I = SHAPES[name] if name in SHAPES else (1, 5)
        _CASES[name] = _Case(B, I, 11 + len(_CASES))
    return _CASES[name]


def cat_prep(c, noise_mode, drop_mode, seed=77, offset=3, coeffs=True, p=0.5):
    lib = _lib.load()
    xin = torch.full((c.B, c.ld), 7.0, device=DEV)  # (stale values: the builder must write every column)
    xt = torch.zeros(c.B, c.ldi, device=DEV)
    temb = torch.zeros(c.B, E, device=DEV)
    ca, cb = (c.ca, c.cb) if coeffs else (None, None)
    _lib.check(lib.gdmcf_cat_prep_input_f32(
        c.x0.data_ptr(), c.x0.stride(0), c.xU.data_ptr(), c.xU.stride(0), c.ts.data_ptr(), _lib.ptr(ca), _lib.ptr(cb), noise_mode,
        c.noise.data_ptr() if noise_mode == 1 else None, c.noise.stride(0), drop_mode, c.keep.data_ptr() if drop_mode == 1 else None,
        c.keep.stride(0), p, seed, offset, c.w.data_ptr(), c.c.data_ptr(), c.emb_w.data_ptr(), c.emb_b.data_ptr(), E, c.B, c.I,
        xin.data_ptr(), xin.stride(0), xt.data_ptr(), xt.stride(0), temb.data_ptr(), _lib.stream_ptr()))
    return xin, xt, temb


def plain_prep(c, noise_mode, drop_mode, seed=77, offset=3, p=0.5):
    """The plain DNN builder on the same rows: its x_t, its xin and temb."""
    lib = _lib.load()
    xin = torch.full((c.B, c.ld), 7.0, device=DEV)
    xt = torch.zeros(c.B, c.ldi, device=DEV)
    temb = torch.zeros(c.B, E, device=DEV)
    _lib.check(lib.gdmcf_dnn_prep_input_f32(
        c.x0.data_ptr(), c.x0.stride(0), c.ts.data_ptr(), c.ca.data_ptr(), c.cb.data_ptr(), noise_mode,
        c.noise.data_ptr() if noise_mode == 1 else None, c.noise.stride(0), drop_mode, c.keep.data_ptr() if drop_mode == 1 else None,
        c.keep.stride(0), p, seed, offset, 0, c.emb_w.data_ptr(), c.emb_b.data_ptr(), E, c.B, c.I, xin.data_ptr(), xin.stride(0),
        xt.data_ptr(), xt.stride(0), temb.data_ptr(), None, _lib.stream_ptr()))
    return xin, xt, temb


def mix_f32(c, xt):
    """The documented order in float32 torch operations on the GPU (each one rounded): ((w0 x_t + w1 u0) + w2 u1) + c."""
    u = c.xU.view(c.B, c.I, 2)
    t = c.w[0, 0] * xt
    t = t + c.w[0, 1] * u[..., 0]
    t = t + c.w[0, 2] * u[..., 1]
    return t + c.c[0]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cat_builder_matches_float32_evaluation(shape):
    """Given noise and keep-mask: x_t and xin[:, :I] equal the float32 torch evaluation bit for bit (the documented order has
    no fused operation, p = 0.5 scales exactly); the columns behind I are the plain builder's, bit for bit."""
    c = case_of(shape)
    I = c.I
    xin, xt, temb = cat_prep(c, 1, 1)
    xt_ref = c.ca[c.ts][:, None] * c.x0 + c.cb[c.ts][:, None] * c.noise
    assert torch.equal(xt[:, :I], xt_ref)
    z = mix_f32(c, xt_ref)
    assert torch.equal(xin[:, :I], torch.where(c.keep != 0, z * 2.0, torch.zeros_like(z)))
    pxin, pxt, ptemb = plain_prep(c, 1, 1)
    assert torch.equal(xt, pxt) and torch.allclose(temb, ptemb, rtol=1e-6, atol=1e-7)
    # behind I: the embedding columns (gdmcf_dnn_emb_cols_f32's dot products), then the plain builder's 1 and zero padding
    assert torch.allclose(xin[:, I:I + E], pxin[:, I:I + E], rtol=1e-6, atol=1e-7)
    assert torch.equal(xin[:, I + E:], pxin[:, I + E:]) and bool((xin[:, I + E] == 1).all()) and bool((xin[:, I + E + 1:] == 0).all())
    # evaluation mode: no dropout, z unscaled; no coefficients: x_t = x0
    xin_e, xt_e, _ = cat_prep(c, 0, 0, coeffs=False)
    assert torch.equal(xt_e[:, :I], c.x0) and torch.equal(xin_e[:, :I], mix_f32(c, c.x0))
    assert torch.allclose(xin_e[:, I:], pxin[:, I:], rtol=1e-6, atol=1e-7) and torch.equal(xin_e[:, I + E:], pxin[:, I + E:])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_cat_builder_philox_draws_are_the_plain_builders(shape):
    """In-kernel noise and dropout with equal (seed, offset): x_t is the plain builder's bit for bit, and so is the keep
    pattern (both dropout inputs are non-zero: noise resp. the cat layer's bias); another offset draws anew."""
    c = case_of(shape)
    I = c.I
    xin, xt, _ = cat_prep(c, 2, 2, seed=1234, offset=9)
    pxin, pxt, _ = plain_prep(c, 2, 2, seed=1234, offset=9)
    assert torch.equal(xt, pxt)
    kept = xin[:, :I] != 0
    assert torch.equal(kept, pxin[:, :I] != 0) and 0.4 < float(kept.float().mean()) < 0.6
    assert torch.equal(xin[:, :I], torch.where(kept, mix_f32(c, xt[:, :I]) * 2.0, torch.zeros_like(xin[:, :I])))
    xin2, xt2, _ = cat_prep(c, 2, 2, seed=1234, offset=9)
    assert torch.equal(xin, xin2) and torch.equal(xt, xt2)
    xin3, xt3, _ = cat_prep(c, 2, 2, seed=1234, offset=10)
    assert not torch.equal(xt, xt3) and not torch.equal(xin3[:, :I] != 0, kept)


# ---- the gradient kernel alone ----------------------------------------------------------------------------------------------
def cat_grad(c, xt, drop_mode, keep=None, seed=77, offset=3, p=0.5):
    lib = _lib.load()
    n = int(lib.gdmcf_cat_grad_ws_bytes(c.B, c.I))
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    gw, gb = torch.zeros(1, 3, device=DEV), torch.zeros(1, device=DEV)
    _lib.check(lib.gdmcf_cat_grad_f32(c.dxin.data_ptr(), c.dxin.stride(0), xt.data_ptr(), xt.stride(0), c.xU.data_ptr(),
                                      c.xU.stride(0), drop_mode, _lib.ptr(keep), keep.stride(0) if keep is not None else 0, p, seed,
                                      offset, c.B, c.I, ws.data_ptr(), n, gw.data_ptr(), gb.data_ptr(), _lib.stream_ptr()))
    return torch.cat([gw.reshape(-1), gb])


@pytest.mark.parametrize("shape", ["wide", "one"])
def test_cat_grad_matches_float64_reduction(shape):
    """The four sums against a float64 torch reduction.  Bound from the kernel's own arithmetic: a float32 product and at most
    16 (thread) + 6 (wave) + 3 (workgroup) float32 additions lie on any term's path before the float64 stage, one rounding
    ends it: |error| <= 26 x 2^-24 x sum |terms| + 2^-24 |sum|.  Two runs give the same bits (no atomics); the keep-mask
    recomputed from the Philox position gives the bits of the same mask handed in."""
    c = case_of(shape)
    I = c.I
    xt = (c.ca[c.ts][:, None] * c.x0 + c.cb[c.ts][:, None] * c.noise).contiguous()
    g = cat_grad(c, xt, 1, c.keep)
    assert torch.equal(g, cat_grad(c, xt, 1, c.keep))
    dz = c.dxin.double() * (c.keep != 0).double() * 2.0
    u = c.xU.view(c.B, I, 2).double()
    terms = [dz * xt.double(), dz * u[..., 0], dz * u[..., 1], dz]
    for k, t in enumerate(terms):
        want, mass = float(t.sum()), float(t.abs().sum())
        err = abs(float(g[k]) - want)
        print(f"{shape} sum {k}: {float(g[k]):.9g} vs {want:.9g} (error {err:.3g}, bound {26 * 2 ** -24 * mass + 2 ** -24 * abs(want):.3g})")
        assert err <= 26 * 2 ** -24 * mass + 2 ** -24 * abs(want), (k, err)
    # no dropout: every term kept, unscaled
    g0 = cat_grad(c, xt, 0)
    want0 = float((c.dxin.double() * xt.double()).sum())
    assert abs(float(g0[0]) - want0) <= 26 * 2 ** -24 * float((c.dxin.double() * xt.double()).abs().sum()) + 2 ** -24 * abs(want0)
    # the builder's drawn mask, recomputed in the backward pass
    xin, _, _ = cat_prep(c, 1, 2, seed=5, offset=8)
    drawn = (xin[:, :I] != 0).to(torch.uint8).contiguous()
    assert torch.equal(cat_grad(c, xt, 2, seed=5, offset=8), cat_grad(c, xt, 1, drawn))


# ---- reverse loop -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SAMPLE_CASES)
def test_dnncat_p_sample_matches_reference(case):
    fx = H.load("dnncat_sample_" + case)
    meta = H.onehot_sample_meta(fx)
    model, diff = gpu_pair(meta, fx)
    model.eval()
    x = cu(torch.from_numpy(fx["x_start"].astype(np.float32)))
    T = meta["T"]
    csr = x.cpu().to_sparse_csr()
    crow, ccol = cu(csr.crow_indices()), cu(csr.col_indices().to(torch.int32))

    def same_topk(got, want):
        a = gdmcf_amd.masked_topk(got, 10, crow, ccol).cpu()
        b = gdmcf_amd.masked_topk(cu(torch.from_numpy(want)), 10, crow, ccol).cpu()
        return all(set(r.tolist()) == set(s.tolist()) for r, s in zip(a, b))

    p0 = diff.p_sample(model, x, 0, False)
    assert H.relerr(p0.cpu().numpy(), fx["pred_steps0"]) < 2e-5 and same_topk(p0, fx["pred_steps0"])
    pT = diff.p_sample(model, x, T, False, noise0=cu(torch.from_numpy(fx["noise_stepsT"])),
                       sampled0=cu(torch.from_numpy(fx["sampled_stepsT"])))
    assert H.relerr(pT.cpu().numpy(), fx["pred_stepsT"]) < 2e-5 and same_topk(pT, fx["pred_stepsT"])
    cap = {}
    pn = diff.p_sample(model, x, 2, True, noise0=cu(torch.from_numpy(fx["noise_noisy0"])),
                       sampled0=cu(torch.from_numpy(fx["sampled_noisy0"])),
                       step_noise=cu(torch.from_numpy(fx["noise_noisy_steps"])), capture=cap)
    assert H.relerr(pn.cpu().numpy(), fx["pred_noisy"]) < 2e-5 and same_topk(pn, fx["pred_noisy"])
    assert len(cap["mean"]) == T and len(cap["pred_xstart"]) == T  # the fused branch: one posterior epilogue per step
    # x_U as the reference hands it over, [B, I, 2], and flat
    t = torch.zeros(meta["B"], dtype=torch.int64, device=DEV)
    xU, _ = model.engine.onehot_rows(x, None, (x != 0).to(torch.uint8), meta["discrete"])
    with torch.no_grad():
        assert torch.equal(model(x, t, xU), model(x, t, xU.view(meta["B"], meta["I"], 2)))
        with pytest.raises(RuntimeError):
            model(x, t, xU[:, :-2])


# ---- in-kernel randomness -----------------------------------------------------------------------------------------------------
def test_dnncat_rng_path_is_reproducible_from_its_seed():
    """Nothing injected: timesteps, class draws, noise and dropout come from the kernels' Philox streams.  Two runs from one
    seed give identical losses and weights after 3 steps, another seed gives different ones; a batch of device CSR rows is
    densified by training_losses and gives the run of the dense batch."""
    from gdmcf_amd.data_utils import DeviceCSR
    fx = H.load("dnncat_train_ragged_eps_wd")
    meta = H.onehot_train_meta(fx)
    x = torch.from_numpy(fx["s0.x_start"].astype(np.float32))

    def run(seed, sparse=False):
        torch.manual_seed(seed)
        model, diff = gpu_pair(meta, fx)
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.0)
        model.train()
        rows = DeviceCSR(x.numpy(), DEV).batch(torch.arange(meta["B"])) if sparse else cu(x)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = diff.training_losses(model, rows, True)["loss"].mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert np.isfinite(losses).all()
        return losses, [p.detach().clone() for p in model.parameters()]

    la, wa = run(5)
    lb, wb = run(5)
    lc, wc = run(6)
    ld, wd = run(5, sparse=True)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb))
    assert la == ld and all(torch.equal(a, b) for a, b in zip(wa, wd))
    assert la != lc and not all(torch.equal(a, b) for a, b in zip(wa, wc))
    assert not torch.equal(wa[2], cu(H.state_dict_from(fx)["cat_layer.weight"]))  # the cat layer is trained


# ---- the neighbour that shares _onehot_model ---------------------------------------------------------------------------------
def test_dnnonehot_step_still_passes_through_onehot_model():
    fx = H.load("onehot_train_tiny_x0")
    meta = H.onehot_train_meta(fx)
    I, dims = meta["I"], meta["dims"]
    m = gdmcf_amd.DNNOneHot([I] + dims, dims[::-1] + [I], 10)
    m.load_state_dict(H.state_dict_from(fx))
    m = m.to(DEV).train()
    d = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, meta["schedule"], meta["scale"], meta["nmin"], meta["nmax"],
                                            meta["T"], DEV, discrete=meta["discrete"], CatOneHot=True)
    inp = H.onehot_step_inputs(fx, 0)
    terms = d.training_losses(m, cu(inp["x"]), True, ts=cu(inp["ts"]), pt=cu(inp["pt"]), noise=cu(inp["noise"]),
                              drop_mask=cu(inp["drop_mask"]), ts_U=cu(inp["ts_U"]), sampled=cu(inp["sampled"]),
                              drop_mask_U=cu(inp["drop_mask_U"]))
    terms["loss"].mean().backward()
    np.testing.assert_allclose(terms["loss"].detach().cpu().numpy(), fx["s0.loss_vec"], rtol=1e-4, atol=0)
    for k, v in m.named_parameters():
        assert H.relerr(v.grad.cpu().numpy(), fx["g0." + k]) < 2e-4, k
