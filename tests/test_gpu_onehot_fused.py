"""GPU (-m gpu): the optimiser-in-backward on the one-hot backbones (FusedAdamW.fuse_into_backward on DNNOneHot,
DNNOneHotEmbedding, DNNOneHotEmbeddingGCN).  The fused weights are updated by the kernels that form their gradients --
the weight-gradient products' AdamW epilogue for the dense layers, gdmcf_normalize_rows_bwd_adamw_f32 for embedding_item,
gdmcf_scatter_rows_adamw_f32 for embedding_user -- and every result must equal the separate AdamW pass bit for bit."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 5
BACKBONES = ["onehot", "onehot-emb", "onehot-gcn"]
YELP_USERS = 54574


def _model(backbone, I, hid, U, gemm_dtype="f32"):
    if backbone == "onehot":
        return gdmcf_amd.DNNOneHot([I, hid], [hid, I], 10, gemm_dtype=gemm_dtype)
    cls = gdmcf_amd.DNNOneHotEmbedding if backbone == "onehot-emb" else gdmcf_amd.DNNOneHotEmbeddingGCN
    return cls([I, hid], [hid, I], 10, item_num=I, user_num=U, gemm_dtype=gemm_dtype)


def _build(backbone, I, hid, U, gemm_dtype="f32"):
    torch.manual_seed(11)
    m = _model(backbone, I, hid, U, gemm_dtype).to(DEV).train()
    if backbone == "onehot-gcn":
        with torch.no_grad():
            m.sumW.fill_(0.6)  # the GCN branch carries weight
    d = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, DEV, CatOneHot=True)
    d.indexIn = backbone != "onehot"
    o = gdmcf_amd.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    return m, d, o


def _inputs(s, B, I, U, backbone):
    """Injected randomness of step s (drawn on the device: the Yelp-width rows are large)."""
    g = torch.Generator(device=DEV).manual_seed(100 + s)
    r = dict(ts=torch.randint(0, T, (B,), generator=g, device=DEV), pt=torch.ones(B, dtype=torch.float64, device=DEV),
             noise=torch.randn(B, I, generator=g, device=DEV),
             drop_mask=(torch.rand(B, I, generator=g, device=DEV) < 0.5).to(torch.uint8),
             ts_U=torch.randint(0, T, (B,), generator=g, device=DEV),
             sampled=(torch.rand(B, I, generator=g, device=DEV) < 0.02).to(torch.uint8),
             drop_mask_U=(torch.rand(B, 2 * I, generator=g, device=DEV) < 0.5).to(torch.uint8))
    if backbone != "onehot":
        r["index"] = torch.randperm(U, generator=g, device=DEV)[:B].cpu()
    x = (torch.rand(B, I, generator=g, device=DEV) < 0.03).float()
    return x, r


def _steps(m, d, o, backbone, B, I, U, steps, first=0, fused_ids=()):
    losses = []
    for s in range(first, first + steps):
        x, r = _inputs(s, B, I, U, backbone)
        o.zero_grad()
        loss = d.training_losses(m, x, True, **r)["loss"]
        loss.mean().backward()
        for p in m.parameters():
            if id(p) in fused_ids:
                assert p.grad is None
        o.step()
        losses.append(loss.detach().clone())
    return losses


def _run(backbone, I, hid, B, U, fuse, min_numel=1 << 20, gemm_dtype="f32", steps=5):
    m, d, o = _build(backbone, I, hid, U, gemm_dtype)
    if fuse:
        assert o.fuse_into_backward(m, min_numel=min_numel) is o
    m.engine.manual_seed(7)
    losses = _steps(m, d, o, backbone, B, I, U, steps, fused_ids=o._fused_ids)
    torch.cuda.synchronize()
    return m, d, o, losses


def _never_applied(m, backbone):
    return [] if backbone == "onehot" else [p for l in m.out_layers for p in (l.weight, l.bias)]


def _assert_same_run(a, b, backbone):
    (m0, d0, o0, l0), (m1, d1, o1, l1) = a, b
    assert all(torch.equal(x, y) for x, y in zip(l0, l1))
    for (k, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p0, p1), k  # emb_layer included: an emb_bwd that read an already-updated W shows here
        s0, s1 = o0.state.get(p0, {}), o1.state.get(p1, {})
        assert set(s0) - {"_fused_pending"} == set(s1) - {"_fused_pending"}, k
        if s0:
            assert int(s0["step"]) == int(s1["step"]), k
            assert torch.equal(s0["exp_avg"], s1["exp_avg"]), k
            assert torch.equal(s0["exp_avg_sq"], s1["exp_avg_sq"]), k
    for p0, p1 in zip(_never_applied(m0, backbone), _never_applied(m1, backbone)):
        assert len(o0.state.get(p0, {})) == 0 and len(o1.state.get(p1, {})) == 0
    assert torch.equal(d0.Lt_history, d1.Lt_history)


@pytest.mark.parametrize("backbone", BACKBONES)
def test_fused_equals_separate_at_a_ragged_small_shape(backbone):
    """Five steps, every candidate fused (min_numel=1): losses, every parameter, both moments and step counts identical bit for
    bit to the separate pass; fused weights never get a .grad; out_layers of the embedding backbones stay without state."""
    I, hid, B, U = 257, 48, 40, 301
    ref = _run(backbone, I, hid, B, U, fuse=False)
    got = _run(backbone, I, hid, B, U, fuse=True, min_numel=1)
    m, o = got[0], got[2]
    assert o._fused_ids == {id(w) for w in m.fusable_weights()} and m.engine.fused_opt is o
    assert all(w.stride(0) % 32 == 0 for w in m.fusable_weights())
    assert all(int(o.state[w]["step"]) == 5 for w in m.fusable_weights())
    _assert_same_run(ref, got, backbone)


@pytest.mark.parametrize("backbone", BACKBONES)
def test_fused_equals_separate_at_yelp_width(backbone):
    """I = 34 395 items, hid = 1000, a 400-row batch, 54 574 users, default min_numel, seated rows: bit for bit."""
    I, hid, B, U = 34395, 1000, 400, YELP_USERS
    ref = _run(backbone, I, hid, B, U, fuse=False)
    got = _run(backbone, I, hid, B, U, fuse=True)
    m, o = got[0], got[2]
    want = {id(w) for w in m.fusable_weights() if w.numel() >= 1 << 20}
    assert o._fused_ids == want and len(want) >= 3
    if backbone != "onehot":
        assert {id(m.embedding_item.weight), id(m.embedding_user.weight)} <= want
        assert m.embedding_item.weight.stride(0) == 3008 and m.embedding_user.weight.stride(0) == 1024
    _assert_same_run(ref, got, backbone)
    del ref, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("width", ["small", "yelp"])
@pytest.mark.parametrize("backbone", BACKBONES)
def test_fused_in_bf16_mode_equals_separate(backbone, width):
    """gemm_dtype="bf16": the fused products round the same operands the same way and their epilogue applies the same
    element update to the same f32 sums -- bit for bit too, at the small shape and at Yelp width (where the fused entry
    may pick another tile class for the large weights: the reduction over the batch keeps its order)."""
    if width == "small":
        ref = _run(backbone, 257, 48, 40, 301, fuse=False, gemm_dtype="bf16")
        got = _run(backbone, 257, 48, 40, 301, fuse=True, min_numel=1, gemm_dtype="bf16")
    else:
        ref = _run(backbone, 34395, 1000, 400, YELP_USERS, fuse=False, gemm_dtype="bf16", steps=3)
        got = _run(backbone, 34395, 1000, 400, YELP_USERS, fuse=True, gemm_dtype="bf16", steps=3)
    _assert_same_run(ref, got, backbone)
    del ref, got
    torch.cuda.empty_cache()


# ---- the two new kernels through the C ABI ------------------------------------------------------------------------------
HYP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3, grad_scale=1.0)


def _adam64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    g = g * grad_scale
    p = p * (1 - lr * weight_decay)
    m = m * beta1 + (1 - beta1) * g
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - lr / bc1 * m / (v.sqrt() / np.sqrt(bc2) + eps)
    return p, m, v


def _seated(rows, cols, ld, gen, fill=None, positive=False):
    buf = torch.full((rows, ld), 7.0, dtype=torch.float32, device=DEV)  # what lies between the rows must stay untouched
    t = buf[:, :cols]
    x = torch.rand(rows, cols, generator=gen, device=DEV) if positive else torch.randn(rows, cols, generator=gen, device=DEV)
    t.copy_(x * 1e-3 if positive else x * 0.05) if fill is None else t.fill_(fill)
    return buf, t


def _adamw_two_pass(lib, p, g, m, v):
    """gdmcf_adamw_f32 over contiguous copies (the separate pass)."""
    p, g, m, v = (t.contiguous().clone() for t in (p, g, m, v))
    table = torch.tensor([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0]], dtype=torch.int64).to(DEV)
    h = HYP
    _lib.check(lib.gdmcf_adamw_f32(table.data_ptr(), 1, (p.numel() + 4095) // 4096, h["lr"], h["beta1"], h["beta2"], h["eps"],
                                   h["weight_decay"], h["step"], h["grad_scale"], _lib.stream_ptr()))
    torch.cuda.synchronize()
    return p, m, v


def _close64(got, want, rtol, atol):
    err = (got.double() - want).abs()
    return bool((err <= atol + rtol * want.abs()).all())


@pytest.mark.parametrize("D", [3000, 97])
@pytest.mark.parametrize("seated", [False, True])
def test_normalize_rows_bwd_adamw_kernel(D, seated):
    """Every element against the float64 restatement (normalize-backward, then AdamW), bit for bit against the two-pass
    sequence normalize_rows_bwd + adamw, twenty launches bit for bit, padding between seated rows untouched."""
    lib = _lib.load()
    R = 301
    gen = torch.Generator(device=DEV).manual_seed(5)
    ld = (D + 31) // 32 * 32 if seated else D
    X0 = torch.randn(R, D, generator=gen, device=DEV)
    rn = (1.0 / X0.norm(dim=1)).float()
    Y = torch.zeros(R, D + 13, device=DEV)[:, :D]
    Y.copy_(X0 * rn[:, None])  # V / |v| (its own, wider stride)
    dY = torch.randn(R, D, generator=gen, device=DEV) * 1e-3
    Wb, W = _seated(R, D, ld, gen)
    W.copy_(X0)
    mb, m = _seated(R, D, ld, gen)
    vb, v = _seated(R, D, ld, gen, positive=True)
    init = [t.clone() for t in (Wb, mb, vb)]

    def launch():
        for dst, src in zip((Wb, mb, vb), init):
            dst.copy_(src)
        h = HYP
        _lib.check(lib.gdmcf_normalize_rows_bwd_adamw_f32(
            dY.data_ptr(), dY.stride(0), Y.data_ptr(), Y.stride(0), rn.data_ptr(), R, D, W.data_ptr(), W.stride(0), m.data_ptr(),
            v.data_ptr(), h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"], h["grad_scale"],
            _lib.stream_ptr()))
        torch.cuda.synchronize()
        return [t.clone() for t in (Wb, mb, vb)]

    first = launch()
    for _ in range(19):
        assert all(torch.equal(a, b) for a, b in zip(first, launch()))
    if ld > D:
        for b in first:
            assert bool((b[:, D:] == 7.0).all())
    Wg, mg, vg = (b[:, :D] for b in first)
    # float64 restatement
    dY64, Y64, rn64 = dY.double(), Y.double(), rn.double()
    g64 = (dY64 - Y64 * (dY64 * Y64).sum(1, keepdim=True)) * rn64[:, None]
    p64, m64, v64 = _adam64(init[0][:, :D].double(), g64, init[1][:, :D].double(), init[2][:, :D].double(), **HYP)
    gmax = float(g64.abs().max())
    assert _close64(mg, m64, 1e-6, 2e-6 * gmax)
    assert _close64(vg, v64, 1e-5, 1e-12)
    assert _close64(Wg, p64, 3e-7, 1e-8)
    # two-pass: normalize_rows_bwd into a gradient buffer, then the separate AdamW pass
    dX = torch.empty(R, D, device=DEV)
    _lib.check(lib.gdmcf_normalize_rows_bwd_f32(dY.data_ptr(), dY.stride(0), Y.data_ptr(), Y.stride(0), rn.data_ptr(), R, D,
                                                dX.data_ptr(), dX.stride(0), _lib.stream_ptr()))
    p2, m2, v2 = _adamw_two_pass(lib, init[0][:, :D], dX, init[1][:, :D], init[2][:, :D])
    assert torch.equal(Wg, p2) and torch.equal(mg, m2) and torch.equal(vg, v2)


@pytest.mark.parametrize("cols", [1000, 97])
@pytest.mark.parametrize("seated", [False, True])
def test_scatter_rows_adamw_kernel(cols, seated):
    """Every row of the table (rows outside the batch with gradient 0) against the float64 restatement (scatter, then
    AdamW), bit for bit against zeros + scatter_add_rows + adamw, twenty launches bit for bit."""
    lib = _lib.load()
    R, n = 1003, 97  # (R not a multiple of the rows one workgroup owns)
    gen = torch.Generator(device=DEV).manual_seed(6)
    ld = (cols + 31) // 32 * 32 if seated else cols
    lds = cols + 40
    src = torch.randn(n, lds, generator=gen, device=DEV) * 1e-2  # the batch rows sit in a wider buffer (du[:, h12:])
    index = torch.randperm(R, generator=gen, device=DEV)[:n].contiguous()
    Wb, W = _seated(R, cols, ld, gen)
    mb, m = _seated(R, cols, ld, gen)
    vb, v = _seated(R, cols, ld, gen, positive=True)
    init = [t.clone() for t in (Wb, mb, vb)]

    def launch():
        for dst, s in zip((Wb, mb, vb), init):
            dst.copy_(s)
        h = HYP
        _lib.check(lib.gdmcf_scatter_rows_adamw_f32(
            src.data_ptr(), lds, index.data_ptr(), n, R, cols, W.data_ptr(), W.stride(0), m.data_ptr(), v.data_ptr(), h["lr"],
            h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"], h["grad_scale"], _lib.stream_ptr()))
        torch.cuda.synchronize()
        return [t.clone() for t in (Wb, mb, vb)]

    first = launch()
    for _ in range(19):
        assert all(torch.equal(a, b) for a, b in zip(first, launch()))
    if ld > cols:
        for b in first:
            assert bool((b[:, cols:] == 7.0).all())
    Wg, mg, vg = (b[:, :cols] for b in first)
    g64 = torch.zeros(R, cols, dtype=torch.float64, device=DEV)
    g64[index] = src[:, :cols].double()
    p64, m64, v64 = _adam64(init[0][:, :cols].double(), g64, init[1][:, :cols].double(), init[2][:, :cols].double(), **HYP)
    assert _close64(mg, m64, 1e-6, 1e-9)
    assert _close64(vg, v64, 1e-5, 1e-12)
    assert _close64(Wg, p64, 3e-7, 1e-8)
    out = torch.ones(R, dtype=torch.bool, device=DEV)
    out[index] = False
    assert int(out.sum()) == R - n and not torch.equal(Wg[out], init[0][:, :cols][out])  # untouched rows move too
    # two-pass: zeroed dense gradient, scatter_add_rows into it, the separate AdamW pass
    dW = torch.zeros(R, cols, device=DEV)
    _lib.check(lib.gdmcf_scatter_add_rows_f32(src.data_ptr(), lds, index.data_ptr(), n, cols, dW.data_ptr(), dW.stride(0),
                                              _lib.stream_ptr()))
    p2, m2, v2 = _adamw_two_pass(lib, init[0][:, :cols], dW, init[1][:, :cols], init[2][:, :cols])
    assert torch.equal(Wg, p2) and torch.equal(mg, m2) and torch.equal(vg, v2)


# ---- checkpoints and data parallel ----------------------------------------------------------------------------------------
def test_checkpoint_resume_with_fused_one_hot_backbone(tmp_path):
    """DNNOneHotEmbeddingGCN trained fused, checkpointed after two steps: a fresh model / optimiser -- fused before OR after
    loading, or never fused -- continues bit for bit; the saved model part loads into a model that never fuses."""
    from gdmcf_amd import checkpoint
    backbone, I, hid, B, U = "onehot-gcn", 257, 48, 40, 301

    def build(fuse):
        m, d, o = _build(backbone, I, hid, U)
        if fuse:
            o.fuse_into_backward(m, min_numel=1)
        return m, d, o

    m, d, o = build(True)
    m.engine.manual_seed(7)
    _steps(m, d, o, backbone, B, I, U, 2, fused_ids=o._fused_ids)
    checkpoint.save_checkpoint(tmp_path / "ck.pt", m, d, o, epoch=2)
    ref = _steps(m, d, o, backbone, B, I, U, 3, first=2, fused_ids=o._fused_ids)
    for order in ("fuse-then-load", "load-then-fuse", "never-fused"):
        m2, d2, o2 = build(order == "fuse-then-load")
        epoch, _ = checkpoint.load_checkpoint(tmp_path / "ck.pt", m2, d2, o2)
        if order == "load-then-fuse":
            o2.fuse_into_backward(m2, min_numel=1)
        assert epoch == 2
        got = _steps(m2, d2, o2, backbone, B, I, U, 3, first=2, fused_ids=o2._fused_ids)
        assert all(torch.equal(a, b) for a, b in zip(ref, got)), order
        for (k, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
            assert torch.equal(a, b), (order, k)
            sa, sb = o.state.get(a, {}), o2.state.get(b, {})
            assert bool(sa) == bool(sb), (order, k)
            if sa:
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (order, k)
                assert int(sa["step"]) == int(sb["step"]), (order, k)
    sd = torch.load(tmp_path / "ck.pt", weights_only=False)["model"]
    plain = _model(backbone, I, hid, U)
    plain.load_state_dict(sd)
    assert all(p.is_contiguous() for p in plain.parameters())


def _dp_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    from gdmcf_amd.parallel import DataParallelStep
    backbone, I, hid, B, U = "onehot-emb", 257, 48, 40, 301
    m, d, o = _build(backbone, I, hid, U)
    o.fuse_into_backward(m, min_numel=1)
    step = DataParallelStep(d, m, o, force_exchange=True)
    res = dict(exchange=step.exchange, fused_ids=len(o._fused_ids), engine_fused=m.engine.fused_opt is not None,
               contiguous=all(p.is_contiguous() for p in m.parameters()))
    m.engine.manual_seed(7)
    losses, grads = [], []
    for s in range(3):
        x, r = _inputs(s, B, I, U, backbone)
        losses.append(float(step(x, True, **r)))
        step.flush()
        grads.append(all(w.grad is not None for w in m.fusable_weights()))
    torch.cuda.synchronize()
    res.update(losses=losses, grads=grads, params=[p.detach().cpu() for p in m.parameters()])
    torch.save(res, os.path.join(out_dir, "dp.pt"))
    dist.destroy_process_group()


def test_data_parallel_step_runs_the_separate_path_on_a_fused_one_hot_model(tmp_path):
    """DataParallelStep with every collective (a one-rank group) switches the fusion off, as for DNN: contiguous weights, no
    weight updated inside the backward, gradients handed to the exchange -- and the run equals the plain unfused one."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_dp_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / "dp.pt")
    assert res["exchange"] and res["fused_ids"] == 0 and not res["engine_fused"] and res["contiguous"]
    assert all(res["grads"])
    backbone, I, hid, B, U = "onehot-emb", 257, 48, 40, 301
    m, d, o = _build(backbone, I, hid, U)
    m.engine.manual_seed(7)
    ref = [float(l.mean()) for l in _steps(m, d, o, backbone, B, I, U, 3)]
    np.testing.assert_allclose(res["losses"], ref, rtol=1e-6)
    for a, p in zip(res["params"], m.parameters()):
        assert float((a - p.detach().cpu()).abs().max()) <= 1e-6
