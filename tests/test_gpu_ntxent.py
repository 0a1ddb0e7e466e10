"""GPU (-m gpu): the NT-Xent term and its gradient as HIP kernels (csrc/ntxent.hip) -- the two entries alone against float64
autograd of the oracle's expression, then `ntxent="fused"` on the two embedding backbones against the reference's fixtures, the
torch route, the CSR route, bf16 GEMM inputs and the fused optimiser."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType
from gdmcf_amd.data_utils import DeviceCSR
from oracle import gdmcf_oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 1), (5, 7), (64, 64), (65, 100), (130, 1000), (400, 1000), (1024, 1030)]
KINDS = ["mild", "peaked", "anti"]
SCALE = 0.37


def cu(t):
    return t.to(DEV)


def bits_equal(a, b):
    """Same dtype, same shape, same bits (NaNs included)."""
    view = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def make_inputs(kind, B, d):
    g = torch.Generator().manual_seed(1000 * B + d)
    if kind == "mild":
        return torch.tanh(0.05 * torch.randn(B, d, generator=g)), torch.tanh(0.05 * torch.randn(B, d, generator=g))
    if kind == "peaked":  # diagonal S about 25 to 30, off-diagonal mass about 1e-9: catches neg_i formed as 1 - P_ii
        z1 = torch.tanh((2.5 / d) ** 0.5 * torch.randn(B, d, generator=g))
        return z1, z1.clone()
    z1 = torch.tanh((1.0 / d) ** 0.5 * torch.randn(B, d, generator=g))  # anti: the diagonal is the row's smallest entry
    return z1, -z1


@functools.lru_cache(maxsize=None)
def reference(kind, B, d):
    """The inputs, float64 autograd of the oracle's expression (scaled by SCALE), and the relerr of the oracle's own float32
    autograd against it -- computed once per case on the CPU, shared, never modified."""
    z1, z2 = make_inputs(kind, B, d)
    out = {}
    for dt in (torch.float64, torch.float32):
        a, b = z1.to(dt).clone().requires_grad_(True), z2.to(dt).clone().requires_grad_(True)
        loss = O.nt_xent_loss(a, b)
        da, db = torch.autograd.grad(loss, (a, b))
        out[dt] = (float(loss.detach()), (SCALE * da).numpy(), (SCALE * db).numpy())
    l64, d1, d2 = out[torch.float64]
    l32, e1, e2 = out[torch.float32]
    return dict(z1=z1, z2=z2, loss=l64, dz1=d1, dz2=d2, loss32=l32, err32=(H.relerr(e1, d1), H.relerr(e2, d2)))


def grad_bounds(ref):
    """8 x the oracle's own float32 error separates another summation order from a wrong term (1e-2 or more); the floor covers
    cases of a handful of elements, where the oracle's figure is luck."""
    return tuple(max(8 * e, 16 * 2.0 ** -24) for e in ref["err32"])


def device_operands(z1, z2):
    """The two operands as column ranges of one wider buffer whose other columns are NaN (rows are not d apart, and what
    follows a row's d elements must never be read): as `bufs.ucat` holds the activations, with an odd offset."""
    B, d = z1.shape
    buf = torch.full((B, 3 + d + 5 + d + 2), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, 3: 3 + d] = cu(z1)
    buf[:, 8 + d: 8 + 2 * d] = cu(z2)
    return buf[:, 3: 3 + d], buf[:, 8 + d: 8 + 2 * d]


@pytest.mark.parametrize("B,d", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_alone_against_float64(kind, B, d):
    """Loss within 2e-5 |loss64| (the oracle's float32 evaluation stays within 1.1e-7); both gradients, as H.relerr against
    float64 autograd, within max(8 x the oracle's float32 autograd relerr on the same inputs, 16 * 2^-24)."""
    ref = reference(kind, B, d)
    assert 0.04 <= abs(ref["loss"]) <= 20  # (the relative loss bound means something: |loss64| is never near 0)
    a, b = device_operands(ref["z1"], ref["z2"])
    scale = torch.full((1,), SCALE, dtype=torch.float32, device=DEV)
    loss, dz1, dz2 = gdmcf_amd.nt_xent_loss_grad(a, b, scale=scale)
    assert loss.shape == (1,) and loss.dtype == torch.float32 and loss.is_cuda
    assert dz1.shape == dz2.shape == (B, d)
    got = float(loss)
    errs = (H.relerr(dz1.cpu().numpy(), ref["dz1"]), H.relerr(dz2.cpu().numpy(), ref["dz2"]))
    bounds = grad_bounds(ref)
    print(f"ntxent {kind} B={B} d={d}: loss64 {ref['loss']:.9g} kernel {got:.9g} rel {abs(got - ref['loss']) / abs(ref['loss']):.2e} "
          f"(oracle f32 {abs(ref['loss32'] - ref['loss']) / abs(ref['loss']):.2e}); relerr dz1 {errs[0]:.2e} dz2 {errs[1]:.2e} "
          f"(oracle f32 {ref['err32'][0]:.2e} {ref['err32'][1]:.2e})")
    assert abs(got - ref["loss"]) <= 2e-5 * abs(ref["loss"])
    assert errs[0] <= bounds[0] and errs[1] <= bounds[1], (errs, bounds)
    # scale = None is 1; the loss does not depend on it
    loss1, u1, _ = gdmcf_amd.nt_xent_loss_grad(a, b)
    assert bits_equal(loss1, loss) and H.relerr(u1.cpu().numpy() * SCALE, ref["dz1"]) <= bounds[0]


def test_two_runs_give_the_same_bits():
    ref = reference("mild", 400, 1000)
    a, b = device_operands(ref["z1"], ref["z2"])
    scale = torch.full((1,), SCALE, dtype=torch.float32, device=DEV)
    first = gdmcf_amd.nt_xent_loss_grad(a, b, scale=scale)
    again = gdmcf_amd.nt_xent_loss_grad(a, b, scale=scale)
    assert all(bits_equal(x, y) for x, y in zip(first, again))
    assert bool(torch.isfinite(first[0]).all()) and float(first[1].abs().max()) > 0


def test_no_host_synchronisation():
    ref = reference("mild", 130, 1000)
    a, b = device_operands(ref["z1"], ref["z2"])
    scale = torch.full((1,), SCALE, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, dz1, dz2 = gdmcf_amd.nt_xent_loss_grad(a, b, scale=scale)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert abs(float(loss) - ref["loss"]) <= 2e-5 * abs(ref["loss"])
    bounds = grad_bounds(ref)
    assert H.relerr(dz1.cpu().numpy(), ref["dz1"]) <= bounds[0] and H.relerr(dz2.cpu().numpy(), ref["dz2"]) <= bounds[1]


def test_entries_refuse_what_they_do_not_cover():
    z = torch.zeros(4097, 8, dtype=torch.float32, device=DEV)
    with pytest.raises(NotImplementedError):
        gdmcf_amd.nt_xent_loss_grad(z, z)
    with pytest.raises(NotImplementedError):
        gdmcf_amd.nt_xent_loss_grad(z[:1], z[:1])
    with pytest.raises(ValueError):
        gdmcf_amd.nt_xent_loss_grad(z[:8], z[:8, :4])
    with pytest.raises(ValueError):
        gdmcf_amd.nt_xent_loss_grad(z[:8], z[:8], scale=0.5)
    with pytest.raises(RuntimeError):
        gdmcf_amd.nt_xent_loss_grad(z[:8].cpu(), z[:8].cpu())


# ---- the reference's fixtures with ntxent="fused" --------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_x0", "ragged_eps_wd"])
def test_fused_route_matches_the_reference_fixtures(case):
    """The training-step assertions of test_onehot_embedding_backbone_matches_reference (tests/test_gpu_onehot.py) with the
    NT-Xent term and its gradient from the HIP kernels."""
    fx = H.load("onehot_emb_" + case)
    meta = H.onehot_emb_meta(fx)
    I, dims = meta["I"], meta["dims"]
    model = gdmcf_amd.DNNOneHotEmbedding([I] + dims, dims[::-1] + [I], 10, item_num=I, user_num=meta["U"], ntxent="fused")
    model.load_state_dict(H.state_dict_from(fx))
    model = model.to(DEV)
    mt = {"x0": ModelMeanType.START_X, "eps": ModelMeanType.EPSILON}[meta["mean_type"]]
    diff = gdmcf_amd.GaussianDiffusionDiscrete(mt, meta["schedule"], meta["scale"], meta["nmin"], meta["nmax"], meta["T"], DEV,
                                               discrete=meta["discrete"], CatOneHot=True)
    diff.indexIn = True
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    model.train()
    for s in range(meta["n_steps"]):
        inp = H.onehot_step_inputs(fx, s)
        opt.zero_grad()
        terms = diff.training_losses(model, cu(inp["x"]), True, index=torch.from_numpy(fx[f"s{s}.index"]), ts=cu(inp["ts"]),
                                     pt=cu(inp["pt"]), noise=cu(inp["noise"]), drop_mask=cu(inp["drop_mask"]),
                                     ts_U=cu(inp["ts_U"]), sampled=cu(inp["sampled"]), drop_mask_U=cu(inp["drop_mask_U"]))
        loss = terms["loss"].mean()
        loss.backward()
        assert model.engine.last_ntxent_route == "fused"
        assert abs(float(model.engine.last_closs) - float(fx[f"s{s}.closs"])) <= 2e-5 * abs(float(fx[f"s{s}.closs"]))
        np.testing.assert_allclose(terms["loss"].detach().cpu().numpy(), fx[f"s{s}.loss_vec"], rtol=1e-4, atol=0)
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


# ---- GCN backbone: fused against torch route -------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2])
def test_gcn_backbone_fused_route_against_torch_route(layers):
    I, hid, B, T, U = 300, 64, 48, 5, 120
    g = torch.Generator().manual_seed(9)
    steps = []
    for s in range(2):
        steps.append((cu((torch.rand(B, I, generator=g) < 0.06).float()),
                      dict(ts=cu(torch.randint(0, T, (B,), generator=g)), pt=cu(torch.ones(B, dtype=torch.float64)),
                           noise=cu(torch.randn(B, I, generator=g)), drop_mask=cu((torch.rand(B, I, generator=g) < 0.5).float()),
                           ts_U=cu(torch.randint(0, T, (B,), generator=g)), sampled=cu((torch.rand(B, I, generator=g) < 0.05).long()),
                           drop_mask_U=cu((torch.rand(B, 2 * I, generator=g) < 0.5).float()),
                           index=torch.randperm(U, generator=g)[:B])))
    runs = {}
    for route in ("torch", "fused"):
        torch.manual_seed(7)
        m = gdmcf_amd.DNNOneHotEmbeddingGCN([I, hid], [hid, I], 10, item_num=I, user_num=U, gcn_layers=layers, ntxent=route)
        with torch.no_grad():
            m.sumW.fill_(0.4)  # (the GCN branch carries weight)
        m = m.to(DEV).train()
        diff = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, DEV, CatOneHot=True)
        diff.indexIn = True
        opt = gdmcf_amd.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
        rec = []
        for x, r in steps:
            opt.zero_grad()
            diff.training_losses(m, x, True, **r)["loss"].mean().backward()
            assert m.engine.last_ntxent_route == route
            rec.append((float(m.engine.last_closs), {k: None if p.grad is None else p.grad.cpu().numpy().copy()
                                                     for k, p in m.named_parameters()}))
            opt.step()
        runs[route] = rec
    for s, ((ct, gt), (cf, gf)) in enumerate(zip(runs["torch"], runs["fused"])):
        assert np.isfinite(ct) and abs(cf - ct) <= 2e-5 * abs(ct), s
        assert any(v is not None for v in gt.values())
        for k in gt:
            assert (gt[k] is None) == (gf[k] is None), k
            if gt[k] is not None:
                assert H.relerr(gf[k], gt[k]) < 3e-4, (k, s)


# ---- combinations ----------------------------------------------------------------------------------------------------------
def _ragged(U, I, density, seed):
    rng = np.random.default_rng(seed)
    dense = (rng.random((U, I)) < density).astype(np.float32)
    dense[0] = 0.0  # one empty row
    return dense


def test_fused_route_on_csr_rows_equals_dense_rows_bit_for_bit():
    """ntxent="fused" with FusedAdamW.fuse_into_backward: a step on csr.batch(ids) equals the step on csr.rows(ids)."""
    U, I, hid, B = 120, 2051, 48, 37
    dcsr = DeviceCSR(sp.csr_matrix(_ragged(U, I, 0.01, seed=3)), DEV)
    rng = np.random.default_rng(0)
    batches = [torch.from_numpy(np.concatenate([rng.permutation(np.arange(1, U))[: B - 1], [0]]).astype(np.int64)) for _ in range(2)]
    runs = []
    for route in ("dense", "sparse"):
        torch.manual_seed(11)
        model = gdmcf_amd.DNNOneHotEmbedding([I, hid], [hid, I], 10, item_num=I, user_num=U, ntxent="fused").to(DEV).train()
        diff = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, 5, DEV, CatOneHot=True)
        diff.indexIn = True
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
        opt.fuse_into_backward(model, min_numel=1 << 12)
        model.engine.manual_seed(99)
        rec = dict(losses=[], closs=[])
        for ids in batches:
            x = dcsr.batch(ids) if route == "sparse" else dcsr.rows(ids)
            opt.zero_grad()
            terms = diff.training_losses(model, x, True, index=ids)
            terms["loss"].mean().backward()
            assert model.engine.last_ntxent_route == "fused"
            rec["losses"].append(terms["loss"].detach().clone())
            rec["closs"].append(model.engine.last_closs.clone())
            opt.step()
        rec["params"] = [p.detach().clone() for p in model.parameters()]
        bufs = model.engine.buffers(B, torch.device(DEV))
        rec["xU"] = bufs.xU
        runs.append(rec)
    a, b = runs
    assert a["xU"] is not None and b["xU"] is None  # the dense route ran, the sparse one never made the [B, 2I] image
    for la, lb in zip(a["losses"] + a["closs"], b["losses"] + b["closs"]):
        assert bool(torch.isfinite(la).all()) and bits_equal(la, lb)
    for pa, pb in zip(a["params"], b["params"]):
        assert bits_equal(pa, pb)


def test_fused_route_with_bf16_gemm_inputs():
    """gemm_dtype="bf16" changes the activations, not the term: float32 kernels on whatever `bufs.ucat` holds."""
    torch.manual_seed(4)
    I, hid, B, T, U = 1500, 96, 64, 5, 300
    model = gdmcf_amd.DNNOneHotEmbedding([I, hid], [hid, I], 10, item_num=I, user_num=U, gemm_dtype="bf16", ntxent="fused")
    model = model.to(DEV).train()
    diff = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, DEV, CatOneHot=True)
    diff.indexIn = True
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    opt.fuse_into_backward(model, min_numel=1 << 12)
    g = torch.Generator().manual_seed(6)
    x = (torch.rand(B, I, generator=g) < 0.02).float()
    opt.zero_grad()
    terms = diff.training_losses(model, cu(x), True, index=torch.randperm(U, generator=g)[:B])
    bufs = model.engine.buffers(B, torch.device(DEV))
    h, hU = bufs.ucat[:, :hid].double().cpu(), bufs.ucat[:, hid: 2 * hid].double().cpu()
    terms["loss"].mean().backward()
    opt.step()
    assert model.engine.last_ntxent_route == "fused"
    want, got = float(O.nt_xent_loss(h, hU)), float(model.engine.last_closs)
    assert np.isfinite(got) and abs(got - want) <= 2e-5 * abs(want)
    assert bool(torch.isfinite(terms["loss"]).all()) and all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_a_batch_of_one_takes_the_torch_route():
    """B = 1 is outside the kernels' range: the step falls back to the torch route and equals the default model's, bit for bit."""
    I, hid, T, U = 300, 64, 5, 120
    g = torch.Generator().manual_seed(2)
    x = cu((torch.rand(1, I, generator=g) < 0.06).float())
    r = dict(ts=cu(torch.randint(0, T, (1,), generator=g)), pt=cu(torch.ones(1, dtype=torch.float64)),
             noise=cu(torch.randn(1, I, generator=g)), drop_mask=cu((torch.rand(1, I, generator=g) < 0.5).float()),
             ts_U=cu(torch.randint(0, T, (1,), generator=g)), sampled=cu((torch.rand(1, I, generator=g) < 0.05).long()),
             drop_mask_U=cu((torch.rand(1, 2 * I, generator=g) < 0.5).float()), index=torch.tensor([17]))
    out = {}
    for route in ("torch", "fused"):
        torch.manual_seed(7)
        m = gdmcf_amd.DNNOneHotEmbedding([I, hid], [hid, I], 10, item_num=I, user_num=U, ntxent=route).to(DEV).train()
        diff = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, DEV, CatOneHot=True)
        diff.indexIn = True
        terms = diff.training_losses(m, x, True, **r)
        terms["loss"].mean().backward()
        assert m.engine.last_ntxent_route == "torch"
        out[route] = [terms["loss"].detach(), m.engine.last_closs] + [p.grad for p in m.parameters() if p.grad is not None]
    assert len(out["torch"]) == len(out["fused"]) > 2
    assert all(bits_equal(a, b) for a, b in zip(out["torch"], out["fused"]))
