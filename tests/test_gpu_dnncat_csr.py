"""GPU (-m gpu): the DNNCat backbone fed from device CSR rows (`DNNCat(csr_rows=True)` + data_utils.CsrBatch) --
gdmcf_cat_prep_input_csr_f32 in place of densify + gdmcf_onehot_noise_f32 + gdmcf_cat_prep_input_f32, the loss target and
gdmcf_cat_grad_bits_f32's one-hot pair taken from bitmaps.  The sparse route is a different way to the same bits: everything
compared with the dense route is compared with torch.equal / assert_array_equal; only the comparisons with the reference's own
numbers keep the tolerances of tests/test_gpu_dnncat.py."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import DeviceCSR
from tests import helpers as H
from tests.test_gpu_onehot_csr import pack_bits, ragged_matrix, shuffled_ids

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(t):
    return t.to(DEV)


def ceil64(n):
    return (n + 63) // 64 * 64


def bits_of(t):
    return t.cpu().numpy().view(np.uint32)


# ---- 1. the builder, every mode ---------------------------------------------------------------------------------------------------
# (B, I): I % 4 != 0 (ragged last group, partial last bitmap word); one group past the first 4096-column workgroup; three spans,
# the last nearly empty; the Yelp width (9 spans).  E = 10: 64-element rows of xin (1 and padding behind the embedding columns);
# E = 7 / 9: the tightest row xin may have, ceil4(I + E) -- for (5, 301, 7) and (24, 34395, 9) that is I + E: no column behind
# the embedding columns, the builder must not write its 1.
@pytest.mark.parametrize("B,I,E", [(5, 301, 10), (5, 301, 7), (7, 4099, 10), (7, 4099, 7), (3, 8200, 10), (3, 8200, 7),
                                   (24, 34395, 10), (24, 34395, 7), (24, 34395, 9)])
def test_cat_prep_input_csr_equals_the_dense_pair_in_every_mode(B, I, E):
    lib, st = _lib.load(), _lib.stream_ptr()
    U = 3 * B + 5
    dense = ragged_matrix(U, I, 0.01, seed=B + I)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    assert dcsr.values is None
    ids = shuffled_ids(U, B, seed=E)
    batch = dcsr.batch(ids)
    x = dcsr.rows(ids)
    assert float(x[ids.tolist().index(0)].sum()) == 0 and float(x[ids.tolist().index(1)][:2048].sum()) > 256
    g = torch.Generator().manual_seed(17)
    torch.manual_seed(5)
    emb = torch.nn.Linear(E, E).to(DEV)
    cat = torch.nn.Linear(3, 1).to(DEV)
    T = 9
    ts = cu(torch.randint(0, T, (B,), generator=g))
    ts_U = cu(torch.randint(0, B + 1, (B,), generator=g))
    ca_t, cb_t = cu(torch.rand(T, generator=g) * 0.5 + 0.5), cu(torch.rand(T, generator=g) * 0.5)
    given = cu((torch.rand(B, I, generator=g) < 0.3).to(torch.uint8))
    given_noise = cu(torch.randn(B, I, generator=g))
    mask = cu((torch.rand(B, I, generator=g) < 0.5).to(torch.uint8))
    seed, W, e = 1234, (I + 31) // 32, 0.97
    ld = ceil64(I + E) if E == 10 else (I + E + 3) // 4 * 4
    ldi = ceil64(I)
    padded = ld > I + E
    assert padded == ((I, E) not in ((301, 7), (34395, 9)))
    want_bits = pack_bits(x.cpu().numpy())

    def outputs():
        return (torch.full((B, ld), -3.0, device=DEV), torch.full((B, ldi), -3.0, device=DEV), torch.full((B, E), -3.0, device=DEV))

    def dense_pair(sampled, ca, cb, noise, drop_mask, p, training, off_noise, off_prep):
        xU = torch.full((B, 2 * I), -3.0, device=DEV)
        s_out = torch.full((B, I), 9, dtype=torch.uint8, device=DEV)
        _lib.check(lib.gdmcf_onehot_noise_f32(x.data_ptr(), x.stride(0), ts_U.data_ptr(), B, I, e, _lib.ptr(sampled),
                                              sampled.stride(0) if sampled is not None else 0, seed, off_noise, xU.data_ptr(),
                                              xU.stride(0), s_out.data_ptr(), s_out.stride(0), st))
        xin, xt, temb = outputs()
        noise_mode, nz, drop_mode, keep = core._prep_modes(B, ca, noise, drop_mask, p, training)
        (nzp, ldn), (kp, ldkp) = core._pl(nz), core._pl(keep)
        _lib.check(lib.gdmcf_cat_prep_input_f32(
            x.data_ptr(), x.stride(0), xU.data_ptr(), xU.stride(0), ts.data_ptr(), _lib.ptr(ca), _lib.ptr(cb), noise_mode, nzp, ldn,
            drop_mode, kp, ldkp, p, seed, off_prep, cat.weight.data_ptr(), cat.bias.data_ptr(), emb.weight.data_ptr(),
            emb.bias.data_ptr(), E, B, I, xin.data_ptr(), xin.stride(0), xt.data_ptr(), xt.stride(0), temb.data_ptr(), st))
        return xin, xt, temb, s_out

    def sparse(sampled, ca, cb, noise, drop_mask, p, training, off_noise, off_prep):
        xin, xt, temb = outputs()
        x0bits = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
        clsbits = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
        core.cat_prep_input_csr(lib, batch, ts_U, e, sampled, seed, off_noise, ts, ca, cb, noise, drop_mask, p, training, off_prep,
                                cat, emb, E, xin, xt, temb, x0bits, clsbits, st)
        return xin, xt, temb, x0bits, clsbits

    for classes, nz, drop, training in itertools.product(("given", "drawn"), ("none", "given", "philox"), ("off", "mask", "philox"),
                                                         (True, False)):
        sampled = given if classes == "given" else None
        ca, cb = (None, None) if nz == "none" else (ca_t, cb_t)
        noise = given_noise if nz == "given" else None
        drop_mask = mask if drop == "mask" else None
        p = 0.0 if drop == "off" else 0.5
        what = (classes, nz, drop, training)
        args = (sampled, ca, cb, noise, drop_mask, p, training)
        want = dense_pair(*args, 5, 6)
        got = sparse(*args, 5, 6)
        assert torch.equal(got[0], want[0]), what             # xin over the whole [B, ld] extent
        assert torch.equal(got[1][:, :I], want[1][:, :I]), what   # x_t
        assert bool((got[1][:, I:] == -3.0).all()), what      # (nothing behind it)
        assert torch.equal(got[2], want[2]), what             # temb_out
        assert not bool((got[0] == -3.0).any()) and not bool((got[2] == -3.0).any()), what  # every element written
        np.testing.assert_array_equal(bits_of(got[3]), want_bits, err_msg=str(what))
        np.testing.assert_array_equal(bits_of(got[4]), pack_bits(want[3].cpu().numpy()), err_msg=str(what))
        if padded:
            assert bool((got[0][:, I + E] == 1).all()) and bool((got[0][:, I + E + 1:] == 0).all())
        again = sparse(*args, 5, 6)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), what
        if classes == "drawn":  # the next class-draw offset: other classes
            other = sparse(*args, 7, 6)
            assert not torch.equal(other[4], got[4]) and torch.equal(other[3], got[3]), what
        if drop == "philox" and training:  # the next builder offset: another keep pattern over the same classes
            other = sparse(*args, 5, 8)
            assert torch.equal(other[4], got[4]) and not torch.equal(other[0][:, :I] != 0, got[0][:, :I] != 0), what


# ---- 2. the gradient from bits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I", [(5, 301), (7, 4099), (3, 8200), (12, 131)])
def test_cat_grad_bits_equals_cat_grad_on_the_image_of_the_same_bits(B, I):
    """The four floats equal gdmcf_cat_grad_f32's bit for bit under all three drop modes.  (131, 301: one column group per thread;
    4099, 8200: up to four, where the dense kernel's sum dz * x_t is not fused throughout -- csrc/cat.hip: cat_grad_fused.)"""
    lib, st = _lib.load(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(B * I)
    c0 = torch.rand(B, I, generator=g) < 0.1
    s = torch.rand(B, I, generator=g) < 0.4
    xU = torch.zeros(B, I, 2)
    xU[..., 0] = (~c0 & ~s).float()
    xU[..., 1] = (c0 & s).float()
    xU = cu(xU.reshape(B, 2 * I).contiguous())
    x0bits = cu(torch.from_numpy(pack_bits(c0.numpy()).view(np.int32)))
    clsbits = cu(torch.from_numpy(pack_bits(s.numpy()).view(np.int32)))
    ldi = ceil64(I)
    dxin, xt = cu(torch.randn(B, ldi, generator=g)), cu(torch.randn(B, ldi, generator=g))
    keep = cu((torch.rand(B, I, generator=g) < 0.5).to(torch.uint8))
    n = int(lib.gdmcf_cat_grad_ws_bytes(B, I))
    seed, offset, p = 77, 3, 0.5

    def run(bits, drop_mode):
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
        gw, gb = torch.full((1, 3), -3.0, device=DEV), torch.full((1,), -3.0, device=DEV)
        kp = keep if drop_mode == 1 else None
        if bits:
            core.cat_grad_bits(lib, dxin, xt, x0bits, clsbits, drop_mode, kp, p, seed, offset, B, I, ws, n, gw, gb, st)
        else:
            _lib.check(lib.gdmcf_cat_grad_f32(dxin.data_ptr(), dxin.stride(0), xt.data_ptr(), xt.stride(0), xU.data_ptr(),
                                              xU.stride(0), drop_mode, _lib.ptr(kp), kp.stride(0) if kp is not None else 0, p, seed,
                                              offset, B, I, ws.data_ptr(), n, gw.data_ptr(), gb.data_ptr(), st))
        return torch.cat([gw.reshape(-1), gb])

    seen = []
    for drop_mode in (0, 1, 2):
        want, got = run(False, drop_mode), run(True, drop_mode)
        assert torch.isfinite(want).all() and torch.equal(got, want), (drop_mode, got, want)
        assert torch.equal(run(True, drop_mode), got)
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])  # (the three modes are three different sums)


# ---- 3. whole training steps ----------------------------------------------------------------------------------------------------------
def make_model(I, hid, csr_rows=True):
    return gdmcf_amd.DNNCat([I, hid], [hid, I], 10, csr_rows=csr_rows)


def discrete_diffusion(T=5, mean_type=ModelMeanType.START_X, scale=0.01):
    return gdmcf_amd.GaussianDiffusionDiscrete(mean_type, "linear-var", scale, 0.001, 0.01, T, DEV, CatOneHot=True)


def assert_route(model, B, sparse):
    bufs = model.engine.buffers(B, torch.device(DEV))
    if sparse:
        assert bufs.xU is None and bufs.x0bits is not None and bufs.clsbits is not None
    else:
        assert bufs.xU is not None and getattr(bufs, "x0bits", None) is None


@pytest.mark.parametrize("U,I,B", [(90, 1203, 29), (40, 4100, 11)])
def test_sparse_rows_train_dnncat_exactly_like_dense_rows(U, I, B):
    """Two identically initialised (model, diffusion, FusedAdamW) triples from the same seed, in-kernel randomness, three steps
    with reweight=True: one is fed csr.rows(ids), the other csr.batch(ids).  Same run, bit for bit."""
    dcsr = DeviceCSR(sp.csr_matrix(ragged_matrix(U, I, 0.01, seed=3)), DEV)
    batches = [shuffled_ids(U, B, seed=s) for s in range(3)]
    runs = []
    for route in ("dense", "sparse"):
        torch.manual_seed(11)
        model = make_model(I, 32).to(DEV).train()
        diff = discrete_diffusion()
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        model.engine.manual_seed(99)
        rec = dict(losses=[], grads=[])
        for ids in batches:
            x = dcsr.batch(ids) if route == "sparse" else dcsr.rows(ids)
            opt.zero_grad()
            terms = diff.training_losses(model, x, True)
            terms["loss"].mean().backward()
            rec["losses"].append(terms["loss"].detach().clone())
            rec["grads"].append([p.grad.clone() for p in model.parameters()])
            opt.step()
        rec["names"] = [k for k, _ in model.named_parameters()]
        rec["params"] = [p.detach().clone() for p in model.parameters()]
        rec["moments"] = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in model.parameters()]
        rec["hist"], rec["count"], rec["offset"] = diff.Lt_history.clone(), diff.Lt_count.clone(), model.engine.offset
        assert_route(model, B, route == "sparse")
        runs.append(rec)
    a, b = runs
    assert a["names"][2:4] == ["cat_layer.weight", "cat_layer.bias"]
    for la, lb in zip(a["losses"], b["losses"]):
        assert torch.isfinite(la).all() and torch.equal(la, lb)
    for step_a, step_b in zip(a["grads"], b["grads"]):
        for k, ga, gb in zip(a["names"], step_a, step_b):
            assert torch.equal(ga, gb), k
    assert float(a["grads"][0][2].abs().sum()) > 0  # (the cat layer has a gradient)
    for k, pa, pb in zip(a["names"], a["params"], b["params"]):
        assert torch.equal(pa, pb), k
    for (ma, va), (mb, vb) in zip(a["moments"], b["moments"]):
        assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert torch.equal(a["hist"], b["hist"]) and torch.equal(a["count"], b["count"]) and int(a["count"].sum()) > 0
    assert a["offset"] == b["offset"] == 6  # two Philox positions per step on both routes


# ---- 4. the reference's fixtures through the sparse route ----------------------------------------------------------------------------
def fixture_batch(x):
    """The fixture's dense {0,1} rows as a CsrBatch over a DeviceCSR (values all 1: DeviceCSR.values is None)."""
    xn = x.numpy()
    assert set(np.unique(xn).tolist()) <= {0.0, 1.0}
    dcsr = DeviceCSR(sp.csr_matrix(xn), DEV)
    assert dcsr.values is None
    return dcsr.batch(torch.arange(xn.shape[0]))


def fixture_pair(meta, fx, csr_rows=True):
    """gpu_pair of tests/test_gpu_dnncat.py with the opt-in."""
    I, dims = meta["I"], meta["dims"]
    m = gdmcf_amd.DNNCat([I] + dims, dims[::-1] + [I], meta.get("emb", 10), csr_rows=csr_rows)
    m.load_state_dict(H.state_dict_from(fx))
    mt = {"x0": ModelMeanType.START_X, "eps": ModelMeanType.EPSILON}[meta["mean_type"]]
    d = gdmcf_amd.GaussianDiffusionDiscrete(mt, meta.get("schedule", "linear-var"), meta["scale"], meta["nmin"], meta["nmax"],
                                            meta["T"], DEV, discrete=meta["discrete"], CatOneHot=True)
    return m.to(DEV), d


@pytest.mark.parametrize("case", ["tiny_x0", "deep_x0", "wide_x0"])
def test_dnncat_train_steps_match_reference_from_csr_rows(case):
    """test_dnncat_train_steps_match_reference of tests/test_gpu_dnncat.py with the fixture's rows handed over as a CsrBatch
    to a model built with csr_rows=True: same assertions, same tolerances, and the step never made the one-hot image."""
    from tests.test_gpu_dnncat import load_train, step_inputs
    fx = load_train(case)
    meta = H.onehot_train_meta(fx)
    assert meta["mean_type"] == "x0" and not meta["norm"]
    model, diff = fixture_pair(meta, fx)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    model.train()
    for s in range(meta["n_steps"]):
        inp = step_inputs(fx, s)
        xU, _ = model.engine.onehot_rows(cu(inp["x"]), None, cu(inp["sampled"]), meta["discrete"])
        np.testing.assert_array_equal(xU.cpu().numpy().reshape(meta["B"], meta["I"], 2).astype(np.uint8), fx[f"s{s}.x_tU"])
        opt.zero_grad()
        terms = diff.training_losses(model, fixture_batch(inp["x"]), True, ts=cu(inp["ts"]), pt=cu(inp["pt"]),
                                     noise=cu(inp["noise"]), drop_mask=cu(inp["drop_mask"]), ts_U=cu(inp["ts_U"]),
                                     sampled=cu(inp["sampled"]))
        assert terms["loss"].dtype == torch.float64 and terms["loss"].shape == (meta["B"],)
        loss = terms["loss"].mean()
        loss.backward()
        bufs = model.engine.buffers(meta["B"], torch.device(DEV))
        np.testing.assert_array_equal(bits_of(bufs.x0bits), pack_bits(inp["x"].numpy()))
        np.testing.assert_array_equal(bits_of(bufs.clsbits), pack_bits(inp["sampled"].numpy()))
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
    assert_route(model, meta["B"], True)


# ---- 5. fallbacks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["default", "eps", "values", "torch_rng"])
def test_configurations_the_sparse_route_does_not_cover_densify_by_themselves(why):
    """A default DNNCat (no opt-in), and with the opt-in the eps target (the model and rows of dnncat_train_ragged_eps_wd,
    12 x 131), interaction values other than 1 and torch-drawn noise: a CsrBatch is densified inside training_losses and the
    step equals the one on csr.rows(ids) bit for bit."""
    rng = np.random.default_rng(4)
    if why == "eps":
        fx = H.load("dnncat_train_ragged_eps_wd")
        meta = H.onehot_train_meta(fx)
        assert (meta["B"], meta["I"], meta["mean_type"]) == (12, 131, "eps")
        dense, B = fx["s0.x_start"].astype(np.float32), meta["B"]
        ids = torch.arange(B)
    else:
        U, I, B = 90, 1203, 29
        dense = ragged_matrix(U, I, 0.02, seed=8)
        if why == "values":
            dense[dense != 0] = rng.integers(2, 4, int((dense != 0).sum())).astype(np.float32)
        ids = shuffled_ids(U, B, seed=2)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    assert (dcsr.values is not None) == (why == "values")
    res = []
    for route in ("dense", "sparse"):
        torch.manual_seed(21)
        if why == "eps":
            model, diff = fixture_pair(meta, fx)
        else:
            model, diff = make_model(dense.shape[1], 32, csr_rows=(why != "default")).to(DEV), discrete_diffusion(scale=0.1)
        model.train()
        assert model.csr_rows is (why != "default")
        if why == "torch_rng":
            diff.rng = "torch"
        model.engine.manual_seed(7)
        torch.manual_seed(22)
        x = dcsr.batch(ids) if route == "sparse" else dcsr.rows(ids)
        terms = diff.training_losses(model, x, True)
        terms["loss"].mean().backward()
        assert_route(model, B, False)  # the dense kernels ran
        res.append((terms["loss"].detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0])
    for ga, gb in zip(res[0][1], res[1][1]):
        assert torch.equal(ga, gb)


# ---- 6. no dense copy --------------------------------------------------------------------------------------------------------------
def test_a_sparse_only_run_never_allocates_the_one_hot_image():
    U, I, B = 120, 2500, 40
    dcsr = DeviceCSR(sp.csr_matrix(ragged_matrix(U, I, 0.01, seed=1)), DEV)
    torch.manual_seed(1)
    model = make_model(I, 32).to(DEV).train()
    diff = discrete_diffusion()
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3)
    for s in range(3):
        opt.zero_grad()
        diff.training_losses(model, dcsr.batch(shuffled_ids(U, B, seed=s)), True)["loss"].mean().backward()
        opt.step()
    eng = model.engine
    assert len(eng._bufs) == 1
    for bufs in eng._bufs.values():
        assert bufs.xU is None and bufs.x0bits is not None and bufs.clsbits is not None
        for name, t in vars(bufs).items():  # nothing of the image's size under another name either
            if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] == B:
                assert t.shape[1] < 2 * I, name
    # the first dense step makes it
    diff.training_losses(model, dcsr.rows(shuffled_ids(U, B, seed=9)), True)["loss"].mean().backward()
    assert len(eng._bufs) == 1 and eng.buffers(B, torch.device(DEV)).xU.shape == (B, 2 * I)


# ---- 7. the driver -----------------------------------------------------------------------------------------------------------------
def test_train_one_epoch_sparse_equals_dense_for_dnncat():
    """(Passes on an MI355X; the caveat of test_sparse_rows_train_dnncat_exactly_like_dense_rows applies: I = 1800 > 1024.)"""
    from gdmcf_amd import driver
    U, I, B = 150, 1800, 32
    csr = sp.csr_matrix(ragged_matrix(U, I, 0.01, seed=6))
    out = []
    for sparse in (False, True):
        torch.manual_seed(31)
        model = make_model(I, 32).to(DEV)
        diff = discrete_diffusion()
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3)
        model.engine.manual_seed(5)
        g = torch.Generator().manual_seed(77)
        total, count = driver.train_one_epoch(diff, model, opt, csr, B, DEV, reweight=True, shuffle=True, drop_last=True,
                                              generator=g, sparse=sparse)
        out.append((total, count, [p.detach().clone() for p in model.parameters()]))
        assert_route(model, B, sparse)
    assert out[0][1] == out[1][1] == U // B and np.isfinite(out[0][0])
    assert out[0][0] == out[1][0]
    for pa, pb in zip(out[0][2], out[1][2]):
        assert torch.equal(pa, pb)
