"""GPU (-m gpu): the one-hot backbones fed from device CSR rows (data_utils.CsrBatch) -- gdmcf_onehot_prep_input_csr_f32 for the
second branch's input, gdmcf_dnn_prep_input_csr_f32 for the first, the loss target taken from bitmaps.  The sparse route is a
different way to the same bits: everything compared with the dense route is compared with torch.equal / assert_array_equal;
only the comparisons with the reference's own numbers keep the tolerances of tests/test_gpu_onehot.py."""
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from gdmcf_amd import engine_core as core
from gdmcf_amd.data_utils import CsrBatch, DeviceCSR
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(t):
    return t.to(DEV)


def ceil64(n):
    return (n + 63) // 64 * 64


def pack_bits(dense):
    """[B, I] {0,1} rows as uint32 bitmaps, bit c & 31 of word c >> 5 = column c (what the CSR-fed builders write)."""
    B, I = dense.shape
    W = (I + 31) // 32
    padded = np.zeros((B, W * 32), dtype=np.uint8)
    padded[:, :I] = dense != 0
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint32).reshape(B, W)


def ragged_matrix(U, I, density, seed):
    """{0,1} rows with one empty row (0) and one row (1) with > 256 nonzeros inside its first 2048-item span."""
    rng = np.random.default_rng(seed)
    dense = (rng.random((U, I)) < density).astype(np.float32)
    dense[0] = 0.0
    span = min(I, 2048)
    dense[1] = 0.0
    dense[1, rng.permutation(span)[: min(span - 8, 700)]] = 1.0
    assert dense[1, :2048].sum() > 256
    return dense


def shuffled_ids(U, B, seed):
    """B distinct row ids out of U > 2B (gaps), shuffled, rows 0 (empty) and 1 (crowded) among them."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(2, U))[: B - 2]
    ids = np.concatenate([ids, [0, 1]])
    rng.shuffle(ids)
    return torch.from_numpy(ids.astype(np.int64))


# ---- 1. the kernel, every mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I", [(5, 301), (7, 4099), (48, 34395)])
@pytest.mark.parametrize("E", [10, 7])
def test_onehot_prep_input_csr_equals_the_dense_pair_in_every_mode(B, I, E):
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
    ts = cu(torch.randint(0, 9, (B,), generator=g))
    ts_U = cu(torch.randint(0, B + 1, (B,), generator=g))
    given = cu((torch.rand(B, I, generator=g) < 0.3).to(torch.uint8))
    mask = cu((torch.rand(B, 2 * I, generator=g) < 0.5).to(torch.uint8))
    seed, ld, W, e = 1234, ceil64(2 * I + E), (I + 31) // 32, 0.97
    want_bits = pack_bits(x.cpu().numpy())

    def dense_pair(sampled, drop_mask, p, training, off_noise, off_prep):
        xU = torch.full((B, 2 * I), -3.0, device=DEV)
        s_out = torch.full((B, I), 9, dtype=torch.uint8, device=DEV)
        _lib.check(lib.gdmcf_onehot_noise_f32(x.data_ptr(), x.stride(0), ts_U.data_ptr(), B, I, e, _lib.ptr(sampled),
                                              sampled.stride(0) if sampled is not None else 0, seed, off_noise, xU.data_ptr(),
                                              xU.stride(0), s_out.data_ptr(), s_out.stride(0), st))
        xin = torch.full((B, ld), -3.0, device=DEV)
        temb = torch.full((B, E), -3.0, device=DEV)
        core.prep_input(lib, xU, 2 * I, ts, None, None, None, drop_mask, p, training, seed, off_prep, False, emb, E, xin, None,
                        temb, None, st)
        return xin, temb, s_out

    def sparse(sampled, drop_mask, p, training, off_noise, off_prep):
        xin = torch.full((B, ld), -3.0, device=DEV)
        temb = torch.full((B, E), -3.0, device=DEV)
        s_out = torch.full((B, I), 9, dtype=torch.uint8, device=DEV)
        bits = torch.full((B, W), -1, dtype=torch.int32, device=DEV)
        core.onehot_prep_input_csr(lib, batch, ts_U, e, sampled, seed, off_noise, ts, drop_mask, p, training, off_prep, emb, E,
                                   xin, temb, st, sampled_out=s_out, x0bits=bits)
        return xin, temb, s_out, bits

    for classes, drop, training in itertools.product(("given", "drawn"), ("off", "mask", "philox"), (True, False)):
        sampled = given if classes == "given" else None
        drop_mask = mask if drop == "mask" else None
        p = 0.0 if drop == "off" else 0.5
        what = (classes, drop, training)
        want = dense_pair(sampled, drop_mask, p, training, 5, 6)
        got = sparse(sampled, drop_mask, p, training, 5, 6)
        assert torch.equal(got[0], want[0]), what   # xin2 over the whole [B, ld] extent
        assert torch.equal(got[1], want[1]), what   # temb_out
        assert torch.equal(got[2], want[2]), what   # sampled_out
        np.testing.assert_array_equal(got[3].cpu().numpy().view(np.uint32), want_bits, err_msg=str(what))
        if ld > 2 * I + E:  # (2 * 34 395 + 10 is a multiple of 64: no padding there)
            assert bool((got[0][:, 2 * I + E] == 1).all()) and bool((got[0][:, 2 * I + E + 1:] == 0).all())
        again = sparse(sampled, drop_mask, p, training, 5, 6)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), what
        if classes == "drawn":  # the next class-draw offset: other classes
            other = sparse(sampled, drop_mask, p, training, 7, 6)
            assert not torch.equal(other[2], got[2]) and not torch.equal(other[0], got[0]), what
        if drop == "philox" and training:  # the next dropout offset: another mask over the same classes
            other = sparse(sampled, drop_mask, p, training, 5, 8)
            assert torch.equal(other[2], got[2]) and not torch.equal(other[0], got[0]), what


# ---- 2. whole training steps, three backbones -----------------------------------------------------------------------------------
def make_backbone(name, I, hid, U, gemm_dtype="f32", **kw):
    if name == "onehot":
        return gdmcf_amd.DNNOneHot([I, hid], [hid, I], 10, gemm_dtype=gemm_dtype, **kw)
    cls = gdmcf_amd.DNNOneHotEmbedding if name == "onehot-emb" else gdmcf_amd.DNNOneHotEmbeddingGCN
    return cls([I, hid], [hid, I], 10, item_num=I, user_num=U, gemm_dtype=gemm_dtype, **kw)


def discrete_diffusion(name, T=5, mean_type=ModelMeanType.START_X, scale=0.01):
    d = gdmcf_amd.GaussianDiffusionDiscrete(mean_type, "linear-var", scale, 0.001, 0.01, T, DEV, CatOneHot=True)
    d.indexIn = name != "onehot"
    return d


@pytest.mark.parametrize("variant", ["f32", "bf16", "fused"])
@pytest.mark.parametrize("backbone", ["onehot", "onehot-emb", "onehot-gcn"])
def test_sparse_rows_train_the_one_hot_backbones_exactly_like_dense_rows(backbone, variant):
    """Two identically initialised (model, diffusion, FusedAdamW) triples from the same seed, in-kernel randomness, three
    steps with reweight=True: one is fed csr.rows(ids), the other csr.batch(ids).  Same run, bit for bit."""
    U, I, hid, B = 200, 4099, 48, 37
    dense = ragged_matrix(U, I, 0.006, seed=3)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    batches = [shuffled_ids(U, B, seed=s) for s in range(3)]
    runs = []
    for route in ("dense", "sparse"):
        torch.manual_seed(11)
        model = make_backbone(backbone, I, hid, U, gemm_dtype="bf16" if variant == "bf16" else "f32").to(DEV).train()
        diff = discrete_diffusion(backbone)
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        if variant == "fused":
            opt.fuse_into_backward(model, min_numel=1 << 12)
        model.engine.manual_seed(99)
        rec = dict(losses=[], grads=None)
        for s, ids in enumerate(batches):
            x = dcsr.batch(ids) if route == "sparse" else dcsr.rows(ids)
            kw = dict(index=ids) if backbone != "onehot" else {}
            opt.zero_grad()
            terms = diff.training_losses(model, x, True, **kw)
            terms["loss"].mean().backward()
            rec["losses"].append(terms["loss"].detach().clone())
            if s == 0:
                rec["grads"] = [None if p.grad is None else p.grad.clone() for p in model.parameters()]
            opt.step()
        rec["params"] = [p.detach().clone() for p in model.parameters()]
        rec["moments"] = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                          for p in model.parameters() if p in opt.state and "exp_avg" in opt.state[p]]
        rec["hist"], rec["count"] = diff.Lt_history.clone(), diff.Lt_count.clone()
        bufs = model.engine.buffers(B, torch.device(DEV))
        rec["xU"], rec["bits"] = bufs.xU, bufs.x0bits
        runs.append(rec)
    a, b = runs
    assert a["xU"] is not None and a["bits"] is None      # the dense route ran ...
    assert b["xU"] is None and b["bits"] is not None      # ... and the sparse one never made the [B, 2I] image
    for la, lb in zip(a["losses"], b["losses"]):
        assert torch.isfinite(la).all() and torch.equal(la, lb)
    assert len(a["grads"]) == len(b["grads"]) and any(g is not None for g in a["grads"])
    for ga, gb in zip(a["grads"], b["grads"]):
        assert (ga is None) == (gb is None)
        assert ga is None or torch.equal(ga, gb)
    for pa, pb in zip(a["params"], b["params"]):
        assert torch.equal(pa, pb)
    assert len(a["moments"]) == len(b["moments"]) > 0
    for (ma, va), (mb, vb) in zip(a["moments"], b["moments"]):
        assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert torch.equal(a["hist"], b["hist"]) and torch.equal(a["count"], b["count"])
    assert int(a["count"].sum()) > 0


# ---- 3. the reference's fixtures through the sparse route -----------------------------------------------------------------------
FAST_TRAIN, FALLBACK_TRAIN = {"tiny_x0", "deep_x0"}, {"ragged_eps_wd", "norm_eps"}
FAST_EMB, FALLBACK_EMB = {"tiny_x0"}, {"ragged_eps_wd"}


def test_fixture_split_between_fast_path_and_fallback():
    """Which fixtures the sparse fast path covers (x0 target, no F.normalize) is pinned: a fixture change cannot silently
    leave the fast path untested."""
    assert FAST_TRAIN | FALLBACK_TRAIN == set(H.ONEHOT_TRAIN_CASES) and FAST_EMB | FALLBACK_EMB == set(H.ONEHOT_EMB_CASES)
    for case in H.ONEHOT_TRAIN_CASES:
        meta = H.onehot_train_meta(H.load("onehot_train_" + case))
        assert (meta["mean_type"] == "x0" and not meta["norm"]) == (case in FAST_TRAIN), case
    for case in H.ONEHOT_EMB_CASES:
        meta = H.onehot_emb_meta(H.load("onehot_emb_" + case))
        assert (meta["mean_type"] == "x0" and not meta["norm"]) == (case in FAST_EMB), case


def fixture_batch(x):
    """The fixture's dense {0,1} rows as a CsrBatch over a DeviceCSR (values all 1: DeviceCSR.values is None)."""
    xn = x.numpy()
    assert set(np.unique(xn).tolist()) <= {0.0, 1.0}
    dcsr = DeviceCSR(sp.csr_matrix(xn), DEV)
    assert dcsr.values is None
    return dcsr.batch(torch.arange(xn.shape[0]))


def assert_route(model, B, fast):
    bufs = model.engine.buffers(B, torch.device(DEV))
    if fast:
        assert bufs.x0bits is not None and bufs.xU is None
    else:
        assert bufs.x0bits is None and bufs.xU is not None


@pytest.mark.parametrize("case", H.ONEHOT_TRAIN_CASES)
def test_onehot_train_steps_match_reference_from_csr_rows(case):
    """test_onehot_train_steps_match_reference of tests/test_gpu_onehot.py with the fixture's rows handed over as a
    CsrBatch: same assertions, same tolerances."""
    from tests.test_gpu_onehot import gpu_pair
    fx = H.load("onehot_train_" + case)
    meta = H.onehot_train_meta(fx)
    model, diff = gpu_pair(meta, fx)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    model.train()
    for s in range(meta["n_steps"]):
        inp = H.onehot_step_inputs(fx, s)
        opt.zero_grad()
        terms = diff.training_losses(model, fixture_batch(inp["x"]), True, ts=cu(inp["ts"]), pt=cu(inp["pt"]),
                                     noise=cu(inp["noise"]), drop_mask=cu(inp["drop_mask"]), ts_U=cu(inp["ts_U"]),
                                     sampled=cu(inp["sampled"]), drop_mask_U=cu(inp["drop_mask_U"]))
        assert terms["loss"].dtype == torch.float64 and terms["loss"].shape == (meta["B"],)
        loss = terms["loss"].mean()
        loss.backward()
        np.testing.assert_allclose(terms["loss"].detach().cpu().numpy(), fx[f"s{s}.loss_vec"], rtol=1e-4, atol=0)
        assert abs(float(loss.detach()) - float(fx[f"s{s}.loss"])) <= 1e-4 * abs(float(fx[f"s{s}.loss"]))
        if s == 0:
            for k, v in model.named_parameters():
                assert H.relerr(v.grad.cpu().numpy(), fx["g0." + k]) < 2e-4, k
        opt.step()
        np.testing.assert_array_equal(diff.Lt_count.cpu().numpy(), fx[f"s{s}.Lt_count"])
        np.testing.assert_allclose(diff.Lt_history.cpu().numpy(), fx[f"s{s}.Lt_history"], rtol=1e-4, atol=0)
    for k, v in model.named_parameters():
        d = np.abs(v.detach().cpu().numpy() - fx["pN." + k]).max()
        assert d < 0.02 * meta["lr"] * meta["n_steps"], (k, d)
        assert H.relerr(opt.state[v]["exp_avg"].cpu().numpy(), fx["m." + k]) < 2e-4, k
        assert H.relerr(opt.state[v]["exp_avg_sq"].cpu().numpy(), fx["v." + k]) < 4e-4, k
    assert_route(model, meta["B"], case in FAST_TRAIN)


@pytest.mark.parametrize("case", H.ONEHOT_EMB_CASES)
def test_onehot_embedding_backbone_matches_reference_from_csr_rows(case):
    """The training part of test_onehot_embedding_backbone_matches_reference with the rows handed over as a CsrBatch."""
    from tests.test_gpu_onehot import gpu_emb_pair
    fx = H.load("onehot_emb_" + case)
    meta = H.onehot_emb_meta(fx)
    model, diff = gpu_emb_pair(meta, fx)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    model.train()
    for s in range(meta["n_steps"]):
        inp = H.onehot_step_inputs(fx, s)
        opt.zero_grad()
        terms = diff.training_losses(model, fixture_batch(inp["x"]), True, index=torch.from_numpy(fx[f"s{s}.index"]),
                                     ts=cu(inp["ts"]), pt=cu(inp["pt"]), noise=cu(inp["noise"]), drop_mask=cu(inp["drop_mask"]),
                                     ts_U=cu(inp["ts_U"]), sampled=cu(inp["sampled"]), drop_mask_U=cu(inp["drop_mask_U"]))
        loss = terms["loss"].mean()
        loss.backward()
        assert abs(float(model.engine.last_closs) - float(fx[f"s{s}.closs"])) <= 2e-5 * abs(float(fx[f"s{s}.closs"]))
        np.testing.assert_allclose(terms["loss"].detach().cpu().numpy(), fx[f"s{s}.loss_vec"], rtol=1e-4, atol=0)
        assert abs(float(loss.detach()) - float(fx[f"s{s}.loss"])) <= 1e-4 * abs(float(fx[f"s{s}.loss"]))
        if s == 0:
            for k, v in model.named_parameters():
                if k.startswith("out_layers"):
                    assert v.grad is None
                else:
                    assert H.relerr(v.grad.cpu().numpy(), fx["g0." + k]) < 3e-4, k
        opt.step()
        np.testing.assert_array_equal(diff.Lt_count.cpu().numpy(), fx[f"s{s}.Lt_count"])
        np.testing.assert_allclose(diff.Lt_history.cpu().numpy(), fx[f"s{s}.Lt_history"], rtol=1e-4, atol=0)
    for k, v in model.named_parameters():
        d = np.abs(v.detach().cpu().numpy() - fx["pN." + k]).max()
        assert d < 0.02 * meta["lr"] * meta["n_steps"], (k, d)
    assert_route(model, meta["B"], case in FAST_EMB)


# ---- 4. fallbacks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("why", ["values", "norm", "eps", "torch_rng"])
def test_configurations_the_fast_path_does_not_cover_densify_by_themselves(why):
    """Interaction values other than 1, F.normalize, the eps target (and torch-drawn noise): a CsrBatch is densified inside
    training_losses and the step equals the one on csr.rows(ids)."""
    rng = np.random.default_rng(4)
    U, I, hid, B, T = 90, 1203, 32, 29, 5
    dense = ragged_matrix(U, I, 0.02, seed=8)
    if why == "values":
        dense[dense != 0] = rng.integers(1, 4, int((dense != 0).sum())).astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    assert (dcsr.values is not None) == (why == "values")
    ids = shuffled_ids(U, B, seed=2)
    res = []
    for route in ("dense", "sparse"):
        torch.manual_seed(21)
        model = make_backbone("onehot", I, hid, U, norm=(why == "norm")).to(DEV).train()
        diff = discrete_diffusion("onehot", T, ModelMeanType.EPSILON if why == "eps" else ModelMeanType.START_X, scale=0.1)
        if why == "torch_rng":
            diff.rng = "torch"
        model.engine.manual_seed(7)
        torch.manual_seed(22)
        x = dcsr.batch(ids) if route == "sparse" else dcsr.rows(ids)
        terms = diff.training_losses(model, x, True)
        terms["loss"].mean().backward()
        bufs = model.engine.buffers(B, torch.device(DEV))
        assert bufs.x0bits is None and bufs.xU is not None  # the dense kernels ran
        res.append((terms["loss"].detach().clone(), [p.grad.clone() for p in model.parameters()]))
    assert torch.isfinite(res[0][0]).all() and torch.equal(res[0][0], res[1][0])
    for ga, gb in zip(res[0][1], res[1][1]):
        assert torch.equal(ga, gb)


# ---- 5. no dense copy ------------------------------------------------------------------------------------------------------------
def test_a_sparse_only_run_never_allocates_the_one_hot_image():
    U, I, hid, B = 120, 2500, 32, 40
    dcsr = DeviceCSR(sp.csr_matrix(ragged_matrix(U, I, 0.01, seed=1)), DEV)
    torch.manual_seed(1)
    model = make_backbone("onehot-emb", I, hid, U).to(DEV).train()
    diff = discrete_diffusion("onehot-emb")
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3)
    for s in range(3):
        ids = shuffled_ids(U, B, seed=s)
        opt.zero_grad()
        diff.training_losses(model, dcsr.batch(ids), True, index=ids)["loss"].mean().backward()
        opt.step()
    eng = model.engine
    assert len(eng._bufs) == 1
    for bufs in eng._bufs.values():
        assert bufs.xU is None and bufs.x0bits is not None
        for name, t in vars(bufs).items():  # nothing of the image's size under another name either
            if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] == B:
                assert t.shape[1] < 2 * I or name == "xin2", name
    # the first dense step makes it
    ids = shuffled_ids(U, B, seed=9)
    diff.training_losses(model, dcsr.rows(ids), True, index=ids)
    assert eng.buffers(B, torch.device(DEV)).xU.shape == (B, 2 * I)


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------
def test_train_one_epoch_sparse_equals_dense_for_the_index_backbone():
    from gdmcf_amd import driver
    U, I, hid, B = 150, 1800, 32, 32
    csr = sp.csr_matrix(ragged_matrix(U, I, 0.01, seed=6))
    out = []
    for sparse in (False, True):
        torch.manual_seed(31)
        model = make_backbone("onehot-emb", I, hid, U).to(DEV)
        diff = discrete_diffusion("onehot-emb")
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3)
        model.engine.manual_seed(5)
        g = torch.Generator().manual_seed(77)
        total, count = driver.train_one_epoch(diff, model, opt, csr, B, DEV, reweight=True, shuffle=True, drop_last=True,
                                              generator=g, sparse=sparse)
        out.append((total, count, [p.detach().clone() for p in model.parameters()]))
        bufs = model.engine.buffers(B, torch.device(DEV))
        assert (bufs.xU is None) == sparse
    assert out[0][1] == out[1][1] == U // B and np.isfinite(out[0][0])
    assert out[0][0] == out[1][0]
    for pa, pb in zip(out[0][2], out[1][2]):
        assert torch.equal(pa, pb)


def test_csr_batch_is_what_the_loader_yields():
    dcsr = DeviceCSR(sp.csr_matrix(ragged_matrix(40, 300, 0.05, seed=2)), DEV)
    from gdmcf_amd.data_utils import DeviceBatchLoader
    batch, idx = next(iter(DeviceBatchLoader(dcsr, 8, sparse=True)))
    assert isinstance(batch, CsrBatch) and batch.shape == (8, 300) and torch.equal(batch.dense(), dcsr.rows(idx))
