"""GPU (-m gpu): dr_tn_kernel, dr_tn_adamw_kernel (csrc/gemm_dr_tn.hip) and dr_kn_kernel (csrc/gemm_dr_kn.hip) at every ring
depth, update mode and edge the batch row count, the shape and the strides select, through the C ABI.

How the weight-gradient kernels run follows from the batch row count B (dr_tn_prepare; tests/dr_ref.py models it and
tests/test_host_dr_ref.py holds the model to the library): the ring depth D in {7, 8, 9} -- three instantiations with their own wait
counts and stream schedule --, the padded k-steps that read past the operands, a partial last k-step, and whether the fused AdamW
update runs inside the next tile's k loop (>= 9 ring rounds) or at the end of the tile.  Every case asserts its configuration
through gdmcf_debug_dr_tn_plan and its kernel through gdmcf_debug_last_gemm.

Buffers: dZ and A are windows of NaN-filled buffers (NaN beside every row and in 64 rows behind the last one: whatever the buffer
descriptors do not zero in a k tail or a padded step surfaces as NaN), outputs are NaN where the kernel writes and canaries
everywhere else (tests/glue_ref.py: seat / canary_intact).

Gates: every element of dW against the float64 product under dr_ref.product_bound (derived, element-wise); db against float64 with
the tolerance of tests/test_gpu_fullsize.py; the fused entries bit for bit against gdmcf_adamw_f32 applied to the plain entry's dW
from the same state (tests/test_gpu_adamw.py bounds that kernel against float64), and against the float64 update with the
tolerances of test_gpu_fullsize.py::test_fused_adamw_weight_gradient_every_element_against_float64 as a backstop.  Each case prints
its worst error / bound ratio.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import dr_ref as D
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N0, K0 = 1024, 2048  # the sweep's shape: 16 x 32 tiles of 64 x 64, the fewest the kernels take
PAD = 32             # guard columns of a seated output (rows stay on 128-byte lines)
# AdamW scalars of the products of a list: lr, weight_decay, step and grad_scale all differ.  The float64 gate's tolerance is stated
# for the first set; the others keep the step's sensitivity to the gradient, lr / (1 - beta1^step) (1 - beta1) grad_scale
# sqrt(1 - beta2^step) / sqrt(v), at or below the first set's (dr_ref.adam_state), so that the same tolerance holds for them.
HYPERS = (
    dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3, grad_scale=0.5),
    dict(lr=7e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=10, grad_scale=1.0),
    dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=40, grad_scale=0.25),
    dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.02, step=7, grad_scale=0.75),
    dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, step=5, grad_scale=0.125),
)
HYPER_KEYS = ("lr", "beta1", "beta2", "eps", "weight_decay", "step", "grad_scale")


# ---- cases: operands and float64 references, computed once per shape on the host ------------------------------------------------
@functools.lru_cache(maxsize=6)
def _case(B, N, K):
    dZ, A, rs = D.dw_operands(B, N, K)
    ref, absprod = D.product_ref(dZ, A)
    dref = (dZ.astype(np.float64) * rs.astype(np.float64)[:, None]).sum(0)
    c = types.SimpleNamespace(B=B, N=N, K=K, dZ=dZ, A=A, rs=rs, ref=ref, bound=D.product_bound(B, absprod), dref=dref)
    for a in (ref, c.bound, dref):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=4)
def _state(N, K):
    return D.adam_state(N, K)


def _window(data, ld, offset=0, rows_behind=64, col=None):
    """(buf, view): a NaN-filled flat buffer whose [rows, ld] window starts `offset` floats in, `rows_behind` more rows of NaN after
    it; `data` in the window's first columns, `col` (if any) in the column right behind them."""
    rows, width = data.shape
    assert ld >= width + (col is not None)
    buf = torch.full((offset + (rows + rows_behind) * ld + 8,), NAN, device=DEV)
    assert buf.data_ptr() % 128 == 0
    view = buf[offset:offset + rows * ld].view(rows, ld)
    view[:, :width] = torch.from_numpy(data).to(DEV)
    if col is not None:
        view[:, width] = torch.from_numpy(col).to(DEV)
    return buf, view


def _plan(B, N, K, lddz, lda, ldw, bias_col, fused):
    """(taken, depth, ksp, tiles_m, tiles_n, m_fastest, has_bias) of gdmcf_debug_dr_tn_plan"""
    v = [ctypes.c_int(-1) for _ in range(6)]
    taken = _lib.load().gdmcf_debug_dr_tn_plan(B, N, K, lddz, lda, ldw, bias_col, fused, *[ctypes.byref(x) for x in v])
    return (taken,) + tuple(x.value for x in v)


class Call:
    """The buffers of one weight-gradient call (plain: dW; fused: W, exp_avg, exp_avg_sq from _state) and its argument lists."""

    def __init__(self, c, scale_col, fused, lddz=None, lda=None, ldw=None, off=0, hyper=HYPERS[0], share=None):
        self.c, self.scale_col, self.fused, self.off, self.hyper = c, scale_col, fused, off, hyper
        self.lddz, self.lda, self.ldw = lddz or c.N + 8, lda or c.K + 8, ldw or c.K + PAD
        if share is None:
            self.dZ = _window(c.dZ, self.lddz, off)
            self.A = _window(c.A, self.lda, off, col=c.rs if scale_col else None)  # column K: the row scale when claimed, else NaN
            self.rs = torch.from_numpy(c.rs).to(DEV)
            self.out = ([R.seat(c.N, c.K, self.ldw, DEV, x, offset=off) for x in _state(c.N, c.K)] if fused
                        else [R.seat(c.N, c.K, self.ldw, DEV, offset=off)])
        else:  # the same read-only operands, the outputs' initial state copied on the device
            self.dZ, self.A, self.rs = share.dZ, share.A, share.rs
            self.out = []
            for buf, _ in share.out0:
                b = buf.clone()
                self.out.append((b, b[off:off + c.N * self.ldw].view(c.N, self.ldw)[:, :c.K]))
        self.out0 = [(b.clone(), None) for b, _ in self.out] if share is None else None
        self.db = R.seat(1, c.N, c.N, DEV)
        for _, v in self.out + [self.dZ, self.A]:
            assert v.data_ptr() % 128 == 4 * off

    def head(self):
        c = self.c
        return (self.dZ[1].data_ptr(), self.lddz, self.A[1].data_ptr(), self.lda, self.rs.data_ptr(), self.scale_col, c.B, c.N, c.K)

    def entry(self):
        """the arguments of gdmcf_linear_bwd_weight_adamw_f32 / the fields of GdDwAdamw"""
        W, m, v = (x[1].data_ptr() for x in self.out)
        return self.head() + (W, self.ldw, m, v, self.db[1].data_ptr()) + tuple(self.hyper[k] for k in HYPER_KEYS)

    def launch(self, lib):
        if self.fused:
            _lib.check(lib.gdmcf_linear_bwd_weight_adamw_f32(*self.entry(), _lib.stream_ptr()))
        else:
            _lib.check(lib.gdmcf_linear_bwd_weight_f32(*self.head(), self.out[0][1].data_ptr(), self.ldw, self.db[1].data_ptr(), 0,
                                                       _lib.stream_ptr()))

    def plan(self):
        return _plan(self.c.B, self.c.N, self.c.K, self.lddz, self.lda, self.ldw, self.scale_col, self.fused)

    def results(self):
        """[dW] or [W, exp_avg, exp_avg_sq], then db: contiguous copies on the device"""
        return [v.contiguous() for _, v in self.out] + [self.db[1][0].clone()]

    def guards_intact(self):
        c = self.c
        return (all(R.canary_intact(b, c.N, c.K, self.ldw, offset=self.off) for b, _ in self.out)
                and R.canary_intact(self.db[0], 1, c.N, c.N))


def _expected_plan(c, scale_col, m_fastest=None):
    Dp, ksp, _, _, _ = D.dr_tn_plan(c.B)
    tm, tn = D.cdiv(c.N, 64), D.cdiv(c.K + scale_col, 64)
    return (1, Dp, ksp, tm, tn, int(tm <= tn) if m_fastest is None else m_fastest, scale_col)


def _check_db(c, db, what):
    err = float(np.abs(db.cpu().double().numpy() - c.dref).max())
    tol = 2e-6 * float(np.abs(c.dref).max()) * max(1.0, (c.B / 400) ** 0.5)
    assert err <= tol, (what, err, tol)  # (NaN fails too)
    return err / tol


def _separate_adamw(lib, dW, state, hyper):
    """gdmcf_adamw_f32 on contiguous copies of the state with the gradient dW: (W, exp_avg, exp_avg_sq)"""
    p, m, v = (torch.from_numpy(x).to(DEV) for x in state)
    g = dW.contiguous()
    table = torch.tensor([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 0]], dtype=torch.int64, device=DEV)
    _lib.check(lib.gdmcf_adamw_f32(table.data_ptr(), 1, D.cdiv(p.numel(), 4096), *[hyper[k] for k in HYPER_KEYS], _lib.stream_ptr()))
    torch.cuda.synchronize()
    return p, m, v


def _check_fused(lib, c, got, dW_plain, hyper, what):
    """gate 1: bit-identical to the plain entry's dW + gdmcf_adamw_f32; gate 2: the float64 update of the float64 product"""
    state = _state(c.N, c.K)
    sep = _separate_adamw(lib, dW_plain, state, hyper)
    differ = [int((a != b).sum()) for a, b in zip(got[:3], sep)]
    p64, m64, v64 = D.adam64(*((state[0], c.ref) + state[1:]), **hyper)
    W, me, ve = (x.cpu().double().numpy() for x in got[:3])
    e_m, e_v, e_p = (float(np.abs(a - b).max()) for a, b in ((me, m64), (ve, v64), (W, p64)))
    t_m, t_v = 4e-6 * float(np.abs(m64).max()), 4e-6 * float(np.abs(v64).max())
    t_p = 4e-6 * float(np.abs(p64).max()) + 2e-5 * hyper["lr"]
    print(f"fused {what}: W / exp_avg / exp_avg_sq elements that differ from dW + gdmcf_adamw_f32: {differ}; err / tolerance "
          f"against float64: W {e_p / t_p:.3f}, exp_avg {e_m / t_m:.3f}, exp_avg_sq {e_v / t_v:.3f}")
    assert differ == [0, 0, 0], (what, differ)
    assert e_m <= t_m and e_v <= t_v and e_p <= t_p, (what, e_m, t_m, e_v, t_v, e_p, t_p)


def _full_case(B, N, K, scale_col, what, m_fastest=None, hyper=HYPERS[0], **strides):
    """The plain and the fused entry on one case with every gate; returns their results on the host: dW, db, W, exp_avg, exp_avg_sq, db."""
    lib = _lib.load()
    c = _case(B, N, K)
    plain = Call(c, scale_col, 0, **strides)
    assert plain.plan() == _expected_plan(c, scale_col, m_fastest), what
    plain.launch(lib)
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == 2, what
    dW, db = plain.results()
    ratio = D.worst_ratio(dW.cpu().numpy(), c.ref, c.bound)
    db_ratio = _check_db(c, db, what)
    print(f"dW {what}: worst err / bound {ratio:.4f}; db err / tolerance {db_ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    assert plain.guards_intact(), what
    fused = Call(c, scale_col, 1, hyper=hyper, **strides)
    assert fused.plan() == _expected_plan(c, scale_col, m_fastest), what
    fused.launch(lib)
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == 3, what
    got = fused.results()
    _check_db(c, got[3], what + " fused")
    assert fused.guards_intact(), what
    _check_fused(lib, c, got, dW, hyper, what)
    return [t.cpu() for t in (dW, db) + tuple(got)]


# ---- a. the batch sweep ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,scale_col", [(B, s) for B in sorted(D.CASES) for s in (0, 1)])
def test_batch_sweep_plain_and_fused(B, scale_col):
    Dp, ksp, waste, rounds, _ = D.CASES[B]
    assert D.dr_tn_plan(B) == (Dp, ksp, waste, rounds, rounds >= 9)
    _full_case(B, N0, K0, scale_col, f"B={B} D={Dp} rounds={rounds} waste={waste} col={scale_col}")


# ---- b. shape edges --------------------------------------------------------------------------------------------------------------
SHAPES = [(2048, 1024, 1), (1000, 2100, 1), (1024, 2049, 0), (1024, 2049, 1), (1024, 2050, 0), (1024, 2050, 1), (1024, 2051, 0),
          (1024, 2051, 1), (64, 32768, 1), (100, 16400, 1)]


@pytest.mark.parametrize("B", [321, 130])
@pytest.mark.parametrize("N,K,scale_col", SHAPES)
def test_shape_edges(N, K, scale_col, B):
    """!m_fastest at the smallest shape; rows past N in the last row tile; K % 4 = 1, 2, 3 without and with the bias column (inside
    a straddling group; at K % 4 = 3 a group of its own is completed); one and two row tiles (one or two tiles per panel)"""
    m_fastest = 0 if (N, K) == (2048, 1024) else 1
    _full_case(B, N, K, scale_col, f"B={B} N={N} K={K} col={scale_col}", m_fastest=m_fastest)


# ---- c. strides and alignment ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _base(B):
    return _full_case(B, N0, K0, 1, f"B={B} base")


STRIDES = {
    "lddz=N+1": dict(lddz=N0 + 1),
    "lda=K+9": dict(lda=K0 + 9),
    "ldw=K+31": dict(ldw=K0 + 31),              # odd: rows start anywhere, the stream's loads stay in L2 (NTL = false)
    "ldw=round32(K)": dict(ldw=(K0 + 31) // 32 * 32),  # rows on 128-byte lines (NTL = true), no guard columns
    "bases+4B": dict(off=1),                     # dZ, A, dW / W / moments one float past a 128-byte line
}


@pytest.mark.parametrize("B", [321, 130])
@pytest.mark.parametrize("variant", sorted(STRIDES))
def test_strides_and_alignment(variant, B):
    """The entries state no alignment beyond float32's: any leading dimension >= the row, any 4-byte-aligned base.  Same gates, and
    the same bits as with the seated, aligned buffers."""
    got = _full_case(B, N0, K0, 1, f"B={B} {variant}", **STRIDES[variant])
    for name, a, b in zip(("dW", "db", "W", "exp_avg", "exp_avg_sq", "db fused"), got, _base(B)):
        assert torch.equal(a, b), (variant, name)


# ---- d. the list entry, directly -------------------------------------------------------------------------------------------------
#           N,    K, scale_col, ldw
PRODUCTS = [(1024, 2048, 1, 2048 + PAD),  # seated
            (2048, 1024, 0, 1024),        # contiguous, !m_fastest
            (1000, 2100, 1, 2131),        # odd ldw, bias column, rows past N
            (1024, 2048, 0, 2048),
            (2048, 1024, 1, 1024 + PAD)]


@pytest.mark.parametrize("B", [321, 130])
@pytest.mark.parametrize("n", [3, 5])
def test_list_entry_against_single_calls(n, B):
    """Products of one batch with different shapes, leading dimensions and AdamW scalars in one list (five: a launch of four and a
    launch of one): a pending tile that took another product's descriptors or scalars shows against the single calls, bit for bit."""
    lib = _lib.load()
    res = []
    for multi in (True, False):
        calls = [Call(_case(B, N, K), col, 1, ldw=ldw, hyper=HYPERS[i]) for i, (N, K, col, ldw) in enumerate(PRODUCTS[:n])]
        plans = [x.plan() for x in calls]
        assert all(p[0] == 1 and p[1:3] == plans[0][1:3] for p in plans) and [p[5] for p in plans] == [1, 0, 1, 1, 0][:n]
        if multi:
            arr = (_lib.GdDwAdamw * n)(*[_lib.GdDwAdamw(*x.entry()) for x in calls])
            _lib.check(lib.gdmcf_linear_bwd_weight_adamw_multi_f32(ctypes.addressof(arr), n, _lib.stream_ptr()))
        else:
            for x in calls:
                x.launch(lib)
        torch.cuda.synchronize()
        assert lib.gdmcf_debug_last_gemm() == 3
        assert all(x.guards_intact() for x in calls)
        res.append([x.results() for x in calls])
    for i, (a, b) in enumerate(zip(*res)):
        for name, x, y in zip(("W", "exp_avg", "exp_avg_sq", "db"), a, b):
            assert torch.equal(x, y), (i, name, int((x != y).sum()))
    if n == 3:  # and the list's results through the gates of the sweep
        for i, (N, K, col, ldw) in enumerate(PRODUCTS[:n]):
            c = _case(B, N, K)
            plain = Call(c, col, 0, ldw=ldw)
            plain.launch(lib)
            torch.cuda.synchronize()
            assert lib.gdmcf_debug_last_gemm() == 2
            dW = plain.results()[0]
            ratio = D.worst_ratio(dW.cpu().numpy(), c.ref, c.bound)
            print(f"dW B={B} product {i} ({N} x {K}): worst err / bound {ratio:.4f}")
            assert ratio <= 1.0
            _check_db(c, res[0][i][3], f"product {i}")
            _check_fused(lib, c, res[0][i], dW, HYPERS[i], f"B={B} product {i}")


# ---- e. ticket sets --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [0, 1])
def test_forty_launches_back_to_back(fused):
    """Eager launches rotate through 16 ticket-counter sets; a set must be zero again when its launch has drained.  Forty launches
    without a synchronisation between them wrap the sets twice: each computes every tile, bit-identical to the first."""
    lib = _lib.load()
    first = Call(_case(321, N0, K0), 1, fused)
    calls = [first] + [Call(first.c, 1, fused, share=first) for _ in range(39)]
    for x in calls:
        x.launch(lib)
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == 2 + fused
    ref = first.results()
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    for i, x in enumerate(calls[1:]):
        for a, b in zip(x.results(), ref):
            assert torch.equal(a, b), i + 1
    assert first.guards_intact() and calls[-1].guards_intact()


# ---- f. dr_kn_kernel through gdmcf_linear_bwd_input_f32 --------------------------------------------------------------------------
#            M,    N,   K, ldw
KN_CASES = [(75, 4100, 128, 136),   # M % 16 != 0: the row clamp; 257 chunks: a tail of 4, a last split of 7 chunks (odd)
            (80, 4096, 120, 128),   # K < 128: the groups of columns 120 .. 127 are parked
            (150, 5000, 250, 252),  # K % 4 = 2: slab rows of 252, the group that straddles K; a last split of 3 chunks
            (152, 4111, 256, 264)]  # odd lddz, a tail of 15


@pytest.mark.parametrize("M,N,K,ldw", KN_CASES)
def test_input_gradient_on_the_split_k_kernel(M, N, K, ldw):
    """dA = rs (dZ W) (1 - act^2) with dZ and W as windows of NaN (NaN behind dZ's N columns: the chunk that reaches past N must
    zero them; NaN rows behind W).  Bound: the product's, (N + 4) u sum |terms| times the epilogue's factors f = 1 - act^2 <= 1 and
    rs -- the split-K partial sums only shorten the chains, N + 4 counts the two multiplications by rs and f --, plus 4 u rs
    sum |terms| for f itself: act^2 and the difference round with absolute error u / 2 each, whatever f is.
    (At N ~ 4100 this worst-case bound is about one typical term, N^2 u ~ 1: it cannot see a single lost product, but a chunk of
    sixteen run twice or not at all, a row or column taken from elsewhere and anything not finite leave it.)"""
    lib = _lib.load()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng([M, N, K])
    dZ = rng.standard_normal((M, N)).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.01).astype(np.float32)
    rs = (rng.random(M) + 0.5).astype(np.float32)
    act = np.tanh(rng.standard_normal((M, K))).astype(np.float32)
    f = 1.0 - act.astype(np.float64) ** 2
    prod, absprod = D.product_ref(dZ.T, W)
    ref = rs.astype(np.float64)[:, None] * prod * f
    bound = D.U * rs.astype(np.float64)[:, None] * absprod * ((N + 4) * f + 4.0)
    zb, zv = _window(dZ, N + 8, rows_behind=8)
    wb, wv = _window(W, ldw)
    rs_d, act_d = torch.from_numpy(rs).to(DEV), torch.from_numpy(act).to(DEV)
    ab, av = R.seat(M, K, K + 8, DEV)
    ws_bytes = int(lib.gdmcf_linear_ws_bytes(M, N, K))
    ws = torch.full((ws_bytes // 4 + 4096,), R.CANARY, device=DEV)
    _lib.check(lib.gdmcf_linear_bwd_input_f32(zv.data_ptr(), N + 8, wv.data_ptr(), ldw, rs_d.data_ptr(), act_d.data_ptr(), K, 1, M, N, K,
                                              av.data_ptr(), K + 8, ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert lib.gdmcf_debug_last_gemm() == 5
    ratio = D.worst_ratio(av.cpu().numpy(), ref, bound)
    print(f"dA M={M} N={N} K={K}: worst err / bound {ratio:.2e}")
    assert ratio <= 1.0
    assert R.canary_intact(ab, M, K, K + 8)
    # the plan, seen through the workspace: `splits` slabs of M x round4(K) written in their first K columns, nothing behind them;
    # gdmcf_linear_ws_bytes holds the `asked` slabs (it also sizes for the forward product of the same three numbers, so >=)
    splits, cps, asked = D.kn_plan(M, N, K, n_cu)
    ldc = (K + 3) // 4 * 4
    assert asked * M * ldc * 4 + 256 <= ws_bytes
    slabs = ws[:splits * M * ldc].view(splits, M, ldc)[:, :, :K]
    assert bool(torch.isfinite(slabs).all()) and not bool((slabs == R.CANARY).any())
    assert bool((ws[splits * M * ldc:] == R.CANARY).all())
