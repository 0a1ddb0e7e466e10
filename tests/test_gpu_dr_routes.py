"""GPU (-m gpu): the take / decline edge of each direct-to-register f32 kernel (csrc/gemm_dr.h: one take-or-decline function per
kernel file, gd_gemm_dr_launch dispatches) and the state of the call around it, through the C ABI.

For every kernel the smallest shape it takes and the nearest shapes it declines (which then run on the LDS-tiled kernel of
csrc/gemm_f32.hip): gdmcf_debug_last_gemm() names the kernel that served the call (2 dr_tn_kernel, 3 dr_tn_adamw_kernel,
4 dr_fat_kernel, 5 dr_kn_kernel, 1 LDS-tiled), and EVERY output element is compared with a float64 host product, tolerance as
tests/test_gpu_fullsize.py (2e-5 of max|ref|, absolute).  A declined call must leave no trace of the attempt: the weight-gradient
kernels widen the product by one column for the bias gradient (GdGemm::N + 1) before they know whether they take it, so the
outputs carry guard columns that must stay untouched, and db must be right whichever pass produced it.

Shapes follow from the predicates (symbols as in gdmcf_linear_bwd_weight_f32: batch M, dW[N, K]):
  dr_tn*:  cdiv(N, 64) * cdiv(K, 64) >= 512 tiles and M >= 128       -> N = 1024, K = 2048 (512), M = 128 | M = 127 | K = 1984 (496)
  dr_kn:   reduction >= 4096, M within 12 % of a multiple of 80      -> M = 80, N = 4096, K = 128        | N = 4080
  dr_fat:  K >= 256; at 256 CUs 5 x cdiv(N, 128) >= 512 tiles        -> M = 400, N = 13184, K = 256      | K = 240 | N = 13056
"""
import ctypes
import functools

import pytest
import torch

from gdmcf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_DW, PAD = 1024, 32  # PAD: guard columns beside dW / W / the moments (rows stay on 128-byte lines)
DW_SHAPES = [(128, 2048, True), (127, 2048, False), (128, 1984, False)]  # batch M, K, taken
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=3, gs=0.5)


def _assert_close(got, ref, what):
    """every element, 2e-5 of max|ref| absolute; `ref` is float64 on the host"""
    err = float((got.detach().cpu().double() - ref).abs().max())
    tol = 2e-5 * float(ref.abs().max())
    print(f"{what}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (what, err, tol)


@functools.lru_cache(maxsize=None)
def _dw_case(M, K):
    """Operands of dW[N, K] = dZ[M, N]^T A[M, K] with the float64 references (computed once per shape, never modified)."""
    g = torch.Generator(device="cpu").manual_seed(M + K)
    dZ = torch.randn(M, N_DW, generator=g) * 0.1
    A = torch.randn(M, K, generator=g)
    rs = torch.rand(M, generator=g) + 0.5
    ref = dZ.double().t() @ A.double()
    dref = (dZ.double() * rs.double()[:, None]).sum(0)
    return dZ.to(DEV), A.to(DEV), rs.to(DEV), ref, dref


def _operand(A, rs, scale_col):
    """A with room behind its K columns (lda > K): column K holds the row scale when the caller says so, something else otherwise"""
    M, K = A.shape
    op = torch.zeros(M, K + 8, device=DEV)
    op[:, :K] = A
    op[:, K] = rs if scale_col else 123.0
    return op


@pytest.mark.parametrize("scale_col", [0, 1])
@pytest.mark.parametrize("M,K,taken", DW_SHAPES)
def test_plain_weight_gradient_taken_and_declined(M, K, taken, scale_col):
    lib = _lib.load()
    dZ, A, rs, ref, dref = _dw_case(M, K)
    op = _operand(A, rs, scale_col)
    dW = torch.full((N_DW, K + PAD), float("nan"), device=DEV)
    db = torch.full((N_DW + 1,), float("nan"), device=DEV)
    _lib.check(lib.gdmcf_linear_bwd_weight_f32(dZ.data_ptr(), N_DW, op.data_ptr(), K + 8, rs.data_ptr(), scale_col, M, N_DW, K,
                                               dW.data_ptr(), K + PAD, db.data_ptr(), 0, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == (2 if taken else 1)
    _assert_close(dW[:, :K], ref, "dW")
    _assert_close(db[:N_DW], dref, "db")
    # exactly N x K elements of dW and N of db written: nothing of the product's extra column beside them
    assert bool(torch.isnan(dW[:, K:]).all()) and bool(torch.isnan(db[N_DW:]).all())


def _adam_state(M, K):
    g = torch.Generator(device="cpu").manual_seed(7 * M + K)
    W0 = torch.randn(N_DW, K, generator=g) * 0.05
    m0 = torch.randn(N_DW, K, generator=g) * 0.01
    v0 = torch.rand(N_DW, K, generator=g) * 1e-3
    return W0, m0, v0


def _adam_ref(gref, W0, m0, v0):
    lr, b1, b2, eps, wd, step, gs = (ADAM[k] for k in ("lr", "b1", "b2", "eps", "wd", "step", "gs"))
    gref = gref * gs
    p = W0.double() * (1 - lr * wd)
    m = m0.double() + (gref - m0.double()) * (1 - b1)
    v = v0.double() * b2 + (1 - b2) * gref * gref
    p = p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    return p, m, v


def _padded(t):
    """t in the first columns of a NaN-filled buffer with PAD guard columns"""
    buf = torch.full((t.shape[0], t.shape[1] + PAD), float("nan"), device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf


def _adam_entry(dZ, op, rs, scale_col, M, K, W, me, ve, db):
    return (dZ.data_ptr(), N_DW, op.data_ptr(), K + 8, rs.data_ptr(), scale_col, M, N_DW, K, W.data_ptr(), K + PAD, me.data_ptr(),
            ve.data_ptr(), db.data_ptr(), ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], ADAM["wd"], ADAM["step"], ADAM["gs"])


@pytest.mark.parametrize("scale_col", [0, 1])
@pytest.mark.parametrize("M,K,taken", DW_SHAPES)
def test_fused_adamw_weight_gradient_taken_and_declined(M, K, taken, scale_col):
    lib = _lib.load()
    dZ, A, rs, ref, dref = _dw_case(M, K)
    op = _operand(A, rs, scale_col)
    W0, m0, v0 = _adam_state(M, K)
    p, m, v = _adam_ref(ref, W0, m0, v0)
    W, me, ve = _padded(W0), _padded(m0), _padded(v0)
    db = torch.full((N_DW + 1,), float("nan"), device=DEV)
    _lib.check(lib.gdmcf_linear_bwd_weight_adamw_f32(*_adam_entry(dZ, op, rs, scale_col, M, K, W, me, ve, db), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == (3 if taken else 1)
    _assert_close(W[:, :K], p, "W")
    _assert_close(me[:, :K], m, "exp_avg")
    _assert_close(ve[:, :K], v, "exp_avg_sq")
    _assert_close(db[:N_DW], dref, "db")
    for t in (W, me, ve):
        assert bool(torch.isnan(t[:, K:]).all())
    assert bool(torch.isnan(db[N_DW:]).all())


def test_fused_adamw_list_with_a_declined_product_falls_back_to_single_calls():
    """gdmcf_linear_bwd_weight_adamw_multi_f32 is all or nothing: one product of the list that dr_tn_adamw_kernel declines sends
    every product through its own call -- nothing launched twice, results bit-identical to those calls."""
    lib = _lib.load()
    outs = []
    for multi in (True, False):
        entries, state = [], []
        for M, K, _ in (DW_SHAPES[0], DW_SHAPES[2]):  # taken, declined (496 tiles)
            dZ, A, rs, _, _ = _dw_case(M, K)
            op = _operand(A, rs, 1)
            W, me, ve = (_padded(t) for t in _adam_state(M, K))
            db = torch.full((N_DW + 1,), float("nan"), device=DEV)
            entries.append(_adam_entry(dZ, op, rs, 1, M, K, W, me, ve, db))
            state += [W, me, ve, db, op]
        if multi:
            arr = (_lib.GdDwAdamw * 2)(*[_lib.GdDwAdamw(*e) for e in entries])
            _lib.check(lib.gdmcf_linear_bwd_weight_adamw_multi_f32(ctypes.addressof(arr), 2, _lib.stream_ptr()))
        else:
            for e in entries:
                _lib.check(lib.gdmcf_linear_bwd_weight_adamw_f32(*e, _lib.stream_ptr()))
        torch.cuda.synchronize()
        assert lib.gdmcf_debug_last_gemm() == 1  # the last product ran on its own, declined
        outs.append(state)
    for a, b in zip(*outs):
        assert torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0))


@pytest.mark.parametrize("N,taken", [(4096, True), (4080, False)])
def test_input_gradient_taken_and_declined(N, taken):
    lib = _lib.load()
    M, K = 80, 128
    g = torch.Generator(device="cpu").manual_seed(N)
    dZ = torch.randn(M, N, generator=g)
    W = torch.randn(N, K, generator=g) * 0.01
    rs = torch.rand(M, generator=g) + 0.5
    act = torch.tanh(torch.randn(M, K, generator=g))
    ref = rs.double()[:, None] * (dZ.double() @ W.double()) * (1 - act.double() ** 2)
    dZ, W, rs, act = dZ.to(DEV), W.to(DEV), rs.to(DEV), act.to(DEV)
    ws = torch.empty(int(lib.gdmcf_linear_ws_bytes(M, N, K)), dtype=torch.uint8, device=DEV)
    dA = torch.full((M, K + PAD), float("nan"), device=DEV)
    _lib.check(lib.gdmcf_linear_bwd_input_f32(dZ.data_ptr(), N, W.data_ptr(), K, rs.data_ptr(), act.data_ptr(), K, 1, M, N, K,
                                              dA.data_ptr(), K + PAD, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == (5 if taken else 1)
    _assert_close(dA[:, :K], ref, "dA")
    assert bool(torch.isnan(dA[:, K:]).all())


def _need_256_cus():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == 256, f"dr_fat_kernel's edge shapes are derived for 256 CUs, this device has {n_cu}"


@functools.lru_cache(maxsize=None)
def _out_layer(N, K):
    M = 400
    g = torch.Generator(device="cpu").manual_seed(N + K)
    h = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    out = h.double() @ W.double().t() + bias.double()
    return h.to(DEV), W.to(DEV), bias.to(DEV), out


@pytest.mark.parametrize("N,K,taken", [(13184, 256, True), (13184, 240, False), (13056, 256, False)])
def test_fused_loss_taken_and_declined(N, K, taken):
    _need_256_cus()
    lib = _lib.load()
    M = 400
    h, W, bias, out = _out_layer(N, K)
    g = torch.Generator(device="cpu").manual_seed(1 + N + K)
    alpha = torch.rand(M, generator=g) + 0.5
    tgt = (torch.rand(M, N, generator=g) < 0.02).float()
    ref = alpha.double()[:, None] * out - tgt.double()
    alpha, tgt = alpha.to(DEV), tgt.to(DEV)
    diff = torch.full((M, N + PAD), float("nan"), device=DEV)
    rowpart = torch.zeros(M * lib.gdmcf_loss_tiles(N), device=DEV)
    rowsum = torch.full((M + 1,), float("nan"), device=DEV)
    _lib.check(lib.gdmcf_linear_loss_fwd_f32(h.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), tgt.data_ptr(), N, alpha.data_ptr(),
                                             M, N, K, None, 0, diff.data_ptr(), N + PAD, rowpart.data_ptr(), rowsum.data_ptr(),
                                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == (4 if taken else 1)
    _assert_close(diff[:, :N], ref, "diff")
    _assert_close(rowsum[:M], (ref * ref).sum(1), "rowsum")
    assert bool(torch.isnan(diff[:, N:]).all()) and bool(torch.isnan(rowsum[M:]).all())


def test_posterior_taken():
    """the reverse step at the fused loss's taken shape: 515 tiles of 80 x 128 fill the LDS-tiled kernel's two rounds of 512
    workgroups to 50 % -- below the 90 % under which dr_fat_kernel takes the posterior"""
    _need_256_cus()
    lib = _lib.load()
    M, N, K = 400, 13184, 256
    h, W, bias, out = _out_layer(N, K)
    g = torch.Generator(device="cpu").manual_seed(2)
    xt = torch.randn(M, N, generator=g)
    c1, c2 = torch.rand(M, generator=g) + 0.2, torch.rand(M, generator=g) + 0.2
    mean = c1.double()[:, None] * out + c2.double()[:, None] * xt.double()
    xt, c1, c2 = xt.to(DEV), c1.to(DEV), c2.to(DEV)
    xn = torch.full((M, N + PAD), float("nan"), device=DEV)
    pred = torch.full((M, N + PAD), float("nan"), device=DEV)
    _lib.check(lib.gdmcf_linear_posterior_fwd_f32(h.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), xt.data_ptr(), N, c1.data_ptr(),
                                                  c2.data_ptr(), None, None, None, None, 0, M, N, K, xn.data_ptr(), N + PAD,
                                                  pred.data_ptr(), N + PAD, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == 4
    _assert_close(pred[:, :N], out, "pred_xstart")
    _assert_close(xn[:, :N], mean, "x_next")
    assert bool(torch.isnan(xn[:, N:]).all()) and bool(torch.isnan(pred[:, N:]).all())
