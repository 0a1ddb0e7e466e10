"""GPU (-m gpu): the dense entries of the C ABI (gdmcf_linear_*) with every fused epilogue and every optional argument, through
each kernel family that can serve them, in all four GEMM modes (f32, bf16, bf16 with registered shadows, f32x3) against float64.

tests/test_gpu_parity.py::test_linear_entry_points_random_shapes walks adversarial shapes through four entries with ONE set of
arguments.  Here: the posterior entry (GD_EPI_POST) with all combinations of its optional arguments, the bitmap-target loss entry
held bit for bit to the dense one, the transposed-weight forward down to its fallbacks, and the arguments the older test never
passes (act=0, bias / alpha / out / rowscale / db NULL, accumulate, a_scale_col).

Conventions (as the older test): A ~ N(0,1), W ~ N(0,1)/sqrt(K), bias ~ N(0,1) from seeded host generators; float64 references
computed on the device; in the bf16 modes the reference multiplies the bfloat16-rounded operands (bf16 x bf16 is exact in f32),
everything the epilogue reads stays f32; f32x3 is held to the f32 reference.  Tolerance max|got - want| <= 1e-5 max(1, max|want|),
row sums rtol 2e-5 / atol 2e-6 max, db rtol = atol = 1e-4.  Every case runs with tight and with padded leading dimensions (+3 on
activations and outputs, +1 on weights); outputs are NaN-filled and their guard columns must still be NaN afterwards; every
call is launched twice and must repeat bit for bit; gdmcf_debug_last_gemm() must name the expected kernel family
(1 LDS-tiled f32, 4 dr_fat, 5 dr_kn, 7 bf16, 8 f32x3, 9 gemm_small).

The tile class inside a family cannot be observed; the class each shape is meant for is listed beside it, derived from
gd_pick_shape_class (gemm_f32.hip) and pick_class(.., fused = true, ..) (linear.hip):
  class 2 (64x64) when M <= 64 or N <= 64, else class 1 (128x128) when 128-row tiles pad at most 3 % worse than 80-row ones,
  else class 0 (80x128); bf16, M > 128: class 3 (208x256) when 208-row tiles pad <= 10 %, at most two row tiles, and -- fused --
  the last round of 256 workgroups is >= 85 % full; f32x3, M > 128 and N >= 128: class 4 (208x128) when 208-row tiles pad <= 10 %.
"""
import contextlib
import functools
import math

import pytest
import torch

from gdmcf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
MODES = ["f32", "bf16", "bf16-shadows", "f32x3"]
PREC = {"f32": 0, "bf16": 1, "bf16-shadows": 1, "f32x3": 2}
MARK = 7.0  # what the shadow of a wider x_next buffer holds beside the N columns the call owns

# (M, N, K) of the fused-epilogue entries and the family code in f32 mode (bf16: 7, f32x3: 8, whatever the shape).
# Tile class in f32 / bf16 / f32x3:
FUSED_SHAPES = [
    ((3, 5, 3), 9),          # K < 4: gemm_small / class 2 / class 2 (the bf16 and f32x3 loaders take K < 4 as it is)
    ((5, 40, 2), 9),         # K < 4: gemm_small / 2 / 2; N is one word plus 8 bits
    ((1, 4, 4), 1),          # M <= 64: 2 / 2 / 2; a single row, N < 32
    ((7, 33, 65), 1),        # M <= 64: 2 / 2 / 2; one word plus one bit
    ((33, 300, 31), 1),      # M <= 64: 2 / 2 / 2; five column tiles, K < one k tile
    ((100, 37, 36), 1),      # N <= 64: 2 / 2 / 2; two row tiles, one word plus 5 bits
    ((100, 257, 36), 1),     # pad128 = 128 <= 1.03 x pad80 = 160: 1 / 1 / 1 (f32x3: M <= 128)
    ((150, 257, 67), 1),     # pad128 = 256 > 1.03 x 160: 0 / 0 (208 pads 39 %) / 0; ragged last row tile, K tail
    ((400, 130, 1000), 1),   # 0 / 0 (2 tiles of a 256-tile round) / 4 (416 pads 4 %, N >= 128); K tail (1000 = 31 x 32 + 8)
    ((65, 64, 8195), 1),     # N <= 64: 2 / 2 / 2; long reduction with a K tail
    ((200, 130, 36), 1),     # 0 / 0 (1 tile of a round) / 4 (208 pads 4 %)
    ((413, 1000, 700), 1),   # 0 / 0 (8 tiles of a round) / 4 (416 pads 0.7 %)
    ((413, 28001, 67), 1),   # 0 / 3 (2 x 110 = 220 tiles >= 85 % of 256) / 4; K < 256 keeps dr_fat away
]
# f32 only: dr_fat_kernel at a ragged N and a K tail.  K >= 256, 5 x cdiv(13190, 128) = 520 tiles of 80 x 128 >= half of the
# 1024 SIMDs (narrowest tile, NB = 8, is the only width that reaches 512); POST: 520 tiles fill two rounds of 512 to 51 % < 90 %.
FAT_SHAPE = ((400, 13190, 259), 4)
FUSED_CASES = [(m, s, c) for m in MODES for s, c in FUSED_SHAPES] + [("f32",) + FAT_SHAPE]
FUSED_IDS = [f"{m}-{s[0]}x{s[1]}x{s[2]}" for m, s, _ in FUSED_CASES]


class _Ctx:
    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode
        self.rounded = mode.startswith("bf16")
        self.shadows = mode == "bf16-shadows"
        self.keep = []

    def code(self, f32_code):
        return {"f32": f32_code, "bf16": 7, "bf16-shadows": 7, "f32x3": 8}[self.mode]

    def shadow(self, t, sync=True):
        sh = _lib.Bf16Shadow(t, sync=sync)
        self.keep.append(sh)
        return sh

    def operand_shadows(self, *ts):
        if self.shadows:
            for t in ts:
                self.shadow(t)

    def release(self):
        """unregister before the allocator can hand the same addresses to new tensors"""
        for sh in self.keep:
            sh.close()
        self.keep = []


@contextlib.contextmanager
def _mode(mode):
    lib = _lib.load()
    prev = lib.gdmcf_gemm_precision(PREC[mode])
    ctx = _Ctx(lib, mode)
    try:
        yield ctx
    finally:
        ctx.release()
        lib.gdmcf_gemm_precision(prev)
        lib.gdmcf_bf16_shadow_clear(None)


def _D(t, rounded):
    return t.bfloat16().double() if rounded else t.double()


def _buf(t, ld, fill=0.0):
    """t in the first columns of a [rows, ld] buffer"""
    b = torch.full((t.shape[0], ld), fill, device=DEV, dtype=t.dtype)
    b[:, :t.shape[1]] = t
    return b


def _close(got, want, what):
    err = float((got.double() - want).abs().max())
    tol = 1e-5 * max(1.0, float(want.abs().max()))
    assert err <= tol, (what, err, tol)  # (a NaN in `got` fails: NaN <= tol is False)


def _close_rows(got, want, what):
    atol = 2e-6 * float(want.abs().max())
    bad = (got.double() - want).abs() > atol + 2e-5 * want.abs()
    assert not bool(bad.any()) and bool(torch.isfinite(got).all()), (what, float((got.double() - want).abs().max()), atol)


def _close_db(got, want, what):
    bad = (got.double() - want).abs() > 1e-4 + 1e-4 * want.abs()
    assert not bool(bad.any()) and bool(torch.isfinite(got).all()), (what, float((got.double() - want).abs().max()))


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    """bit for bit, NaN guards included"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _twice(launch, what):
    """launch() re-initialises its outputs, runs the entry once and returns (family code, clones of every output): run it twice,
    the second result bit-identical to the first"""
    first, second = launch(), launch()
    assert first[0] == second[0], (what, first[0], second[0])
    for a, b in zip(first[1], second[1]):
        assert (a is None and b is None) or _same(a, b), (what, "second launch differs")
    return first


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(1000003 * M + 1009 * N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    return A.to(DEV), W.to(DEV), bias.to(DEV)


@functools.lru_cache(maxsize=None)
def _product(M, N, K, rounded):
    """float64 A W^T (no bias) of the operands as the mode's matrix pipe sees them; computed once, never modified"""
    A, W, _ = _operands(M, N, K)
    return _D(A, rounded) @ _D(W, rounded).t()


def _layer(ctx, M, N, K, pad):
    """(A, lda, W, ldw, bias, float64 A W^T + bias) with the leading dimensions of this pass; shadows registered in shadow mode"""
    A, W, bias = _operands(M, N, K)
    Ab, Wb = _buf(A, K + pad), _buf(W, K + (1 if pad else 0))
    ctx.operand_shadows(Ab[:, :K], Wb[:, :K])
    return Ab, K + pad, Wb, K + (1 if pad else 0), bias, _product(M, N, K, ctx.rounded) + bias.double()


def _each_pad(ctx, case, *args):
    for pad in (0, 3):
        try:
            case(ctx, *args, pad)
        finally:
            ctx.release()


def _route(entry, ctx, shape, pad, code):
    print(f"route {entry} {ctx.mode} {shape[0]}x{shape[1]}x{shape[2]} pad{pad}: family {code}")


# ---- 1. posterior entry ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _posterior_values(M, N):
    g = torch.Generator(device="cpu").manual_seed(7 + 31 * M + N)
    xt, z = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    c1, c2 = torch.rand(M, generator=g) + 0.2, torch.rand(M, generator=g) + 0.2
    r1, r2 = torch.rand(M, generator=g) + 1.0, torch.rand(M, generator=g) * 0.1
    sigma = torch.rand(M, generator=g) * 0.01
    sigma[::3] = 0.0  # the caller zeroes sigma at t == 0
    return tuple(t.to(DEV) for t in (xt, z, c1, c2, r1, r2, sigma))


def _posterior_case(ctx, shape, f32_code, pad):
    """x_next = c1 pred + c2 x_t (+ sigma z), pred = r1 x_t - r2 out or out, out = A W^T + bias (include/gdmcf_hip.h)"""
    lib, (M, N, K) = ctx.lib, shape
    A, lda, W, ldw, bias, out64 = _layer(ctx, M, N, K, pad)
    xt, z, c1, c2, r1, r2, sigma = _posterior_values(M, N)
    xtb, zb = _buf(xt, N + pad, NAN), _buf(z, N + pad, NAN)
    wide = 11 if ctx.shadows else 0  # "x_next lands in a wider xin buffer" (attach_result_shadow)
    xn = torch.empty(M, N + wide + pad, device=DEV)
    pred = torch.empty(M, N + pad, device=DEV)
    sh = ctx.shadow(xn[:, :N + wide], sync=False) if ctx.shadows else None
    col = lambda v: v.double()[:, None]
    got = {}
    for use_r, use_z, use_pred in [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1), (1, 1, 0)]:
        what = ("posterior", ctx.mode, shape, pad, use_r, use_z, use_pred)

        def launch():
            xn.fill_(NAN)
            pred.fill_(NAN)
            if sh is not None:
                sh.buf.zero_()
                sh.buf[:M, N:N + wide] = MARK
            _lib.check(lib.gdmcf_linear_posterior_fwd_f32(
                A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr(), xtb.data_ptr(), N + pad, c1.data_ptr(), c2.data_ptr(),
                r1.data_ptr() if use_r else None, r2.data_ptr() if use_r else None, sigma.data_ptr() if use_z else None,
                zb.data_ptr() if use_z else None, N + pad if use_z else 0, M, N, K, xn.data_ptr(), xn.stride(0),
                pred.data_ptr() if use_pred else None, N + pad if use_pred else 0, _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (xn.clone(), pred.clone(), None if sh is None else sh.buf.clone())

        code, (x, p, s16) = _twice(launch, what)
        _route("posterior", ctx, shape, pad, code)
        assert code == ctx.code(f32_code), (what, code)
        pref = (col(r1) * xt.double() - col(r2) * out64) if use_r else out64
        xref = col(c1) * pref + col(c2) * xt.double()
        if use_z:
            xref = xref + col(sigma) * z.double()
        _close(x[:, :N], xref, what + ("x_next",))
        assert _all_nan(x[:, N:]), what + ("x_next guard columns written",)
        if use_pred:
            _close(p[:, :N], pref, what + ("pred_out",))
            assert _all_nan(p[:, N:]), what + ("pred_out guard columns written",)
        else:
            assert _same(x, got[(use_r, use_z, 1)][0]), what + ("x_next differs without pred_out",)
        if use_z:  # rows with sigma == 0: exactly the mean as computed without z
            rows = sigma == 0
            assert torch.equal(x[rows, :N], got[(use_r, 0, 1)][0][rows, :N]), what + ("sigma == 0 rows differ from the mean",)
        if s16 is not None:
            want16 = torch.zeros_like(s16)
            want16[:M, N:N + wide] = MARK
            want16[:M, :N] = x[:, :N].bfloat16()
            assert _same(s16[:M, :N], want16[:M, :N]), what + ("bf16 shadow of x_next",)
            assert _same(s16, want16), what + ("shadow written outside [M, N]",)
        got[(use_r, use_z, use_pred)] = (x, p)


@pytest.mark.parametrize("mode,shape,f32_code", FUSED_CASES, ids=FUSED_IDS)
def test_posterior_entry(mode, shape, f32_code):
    if f32_code == 4:
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert n_cu == 256, f"dr_fat_kernel's shape is derived for 256 CUs, this device has {n_cu}"
    with _mode(mode) as ctx:
        _each_pad(ctx, _posterior_case, shape, f32_code)


# ---- 2. bitmap loss entry ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _loss_values(M, N):
    g = torch.Generator(device="cpu").manual_seed(11 + 37 * M + N)
    tgt = (torch.rand(M, N, generator=g) < 0.05).float()
    alpha = torch.rand(M, generator=g) + 0.5
    return tgt.to(DEV), alpha.to(DEV)


def _pack_bits(tgt, ldbits):
    """bit n & 31 of word n >> 5 of row m; every bit above column N of the last word and every padding word all ones"""
    M, N = tgt.shape
    nw = (N + 31) // 32
    full = torch.ones(M, nw * 32, dtype=torch.int64, device=DEV)
    full[:, :N] = tgt.long()
    words = (full.view(M, nw, 32) << torch.arange(32, device=DEV)).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    packed = torch.full((M, ldbits), -1, dtype=torch.int32, device=DEV)
    packed[:, :nw] = words
    return packed


def _loss_bits_case(ctx, shape, f32_code, pad):
    lib, (M, N, K) = ctx.lib, shape
    A, lda, W, ldw, bias, out64 = _layer(ctx, M, N, K, pad)
    tgt, alpha = _loss_values(M, N)
    ldbits = (N + 31) // 32 + 2
    packed = _pack_bits(tgt, ldbits)
    tgtb = _buf(tgt, N + pad, NAN)
    nt = lib.gdmcf_loss_tiles(N)
    diff = torch.empty(M, N + pad, device=DEV)
    diff_dense = torch.empty(M, N + pad, device=DEV)
    out = torch.empty(M, N + pad, device=DEV)
    rowpart = torch.empty(M * nt, device=DEV)
    rowsum = torch.empty(M + 1, device=DEV)
    sh = ctx.shadow(diff[:, :N], sync=False) if ctx.shadows else None
    got = {}
    for use_alpha, use_out in [(1, 1), (0, 1), (1, 0)]:
        what = ("loss_bits", ctx.mode, shape, pad, use_alpha, use_out)

        def launch(bits, d):
            def go():
                for t in (d, out, rowsum):
                    t.fill_(NAN)
                rowpart.zero_()
                if sh is not None:
                    sh.buf.zero_()
                common = (alpha.data_ptr() if use_alpha else None, M, N, K, out.data_ptr() if use_out else None,
                          N + pad if use_out else 0, d.data_ptr(), N + pad, rowpart.data_ptr(), rowsum.data_ptr(), _lib.stream_ptr())
                if bits:
                    _lib.check(lib.gdmcf_linear_loss_fwd_bits_f32(A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr(),
                                                                  packed.data_ptr(), ldbits, *common))
                else:
                    _lib.check(lib.gdmcf_linear_loss_fwd_f32(A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr(), tgtb.data_ptr(),
                                                             N + pad, *common))
                code = lib.gdmcf_debug_last_gemm()
                torch.cuda.synchronize()
                return code, (d.clone(), out.clone(), rowsum.clone(), None if sh is None else sh.buf.clone())
            return go

        code, (d, o, rs, s16) = _twice(launch(True, diff), what)
        _route("loss_bits", ctx, shape, pad, code)
        assert code == ctx.code(f32_code), (what, code)
        dref = (alpha.double()[:, None] if use_alpha else 1.0) * out64 - tgt.double()
        _close(d[:, :N], dref, what + ("diff",))
        _close_rows(rs[:M], (dref * dref).sum(1), what + ("rowsum",))
        assert _all_nan(d[:, N:]) and _all_nan(rs[M:]), what + ("guard written",)
        if use_out:
            _close(o[:, :N], out64, what + ("out",))
            assert _all_nan(o[:, N:]), what + ("out guard columns written",)
        else:
            assert _all_nan(o), what + ("out written though NULL",)
            assert _same(d, got[(use_alpha, 1)][0]) and _same(rs, got[(use_alpha, 1)][2]), what + ("diff / rowsum differ without out",)
        if s16 is not None:
            want16 = torch.zeros_like(s16)
            want16[:M, :N] = d[:, :N].bfloat16()
            assert _same(s16[:M, :N], want16[:M, :N]), what + ("bf16 shadow of diff",)
            assert _same(s16, want16), what + ("shadow written outside [M, N]",)
        # the header's promise: bit-identical to the dense entry (same arguments, the target as floats)
        dcode, (dd, do, drs, _) = launch(False, diff_dense)()
        assert dcode == code, (what, "dense entry on family", dcode)
        assert _same(dd, d) and _same(do, o) and _same(drs, rs), what + ("bitmap and dense entry differ",)
        got[(use_alpha, use_out)] = (d, o, rs)


@pytest.mark.parametrize("mode,shape,f32_code", FUSED_CASES, ids=FUSED_IDS)
def test_bitmap_loss_entry(mode, shape, f32_code):
    if f32_code == 4:
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert n_cu == 256, f"dr_fat_kernel's shape is derived for 256 CUs, this device has {n_cu}"
    with _mode(mode) as ctx:
        _each_pad(ctx, _loss_bits_case, shape, f32_code)


# ---- 3. transposed-weight forward --------------------------------------------------------------------------------------

# (M, N, K), family: the product is KC x MC (A[M, K] Wt[K, N]) as split-K slabs; gemm_small when N < 4 or K < 4; dr_kn_kernel
# when K >= 4096, M and N tile by 80 x 128 within 12 % and M >= 16, N >= 64; else LDS-tiled (class from gd_pick_shape_class)
WT_SHAPES = [
    ((2, 3, 3), 9),          # N < 4 and K < 4
    ((5, 2, 9), 9),          # N < 4
    ((17, 33, 65), 1),       # class 2
    ((81, 129, 33), 1),      # class 1
    ((100, 257, 36), 1),     # class 1
    ((7, 1000, 515), 1),     # class 2, split over K
    ((80, 128, 4096), 5),    # dr_kn_kernel: one tile, 32 splits
    ((400, 130, 5000), 1),   # N = 130 pads 128-wide tiles by 97 %: dr_kn declines; class 0, 19 splits
]


def _wt_case(ctx, shape, f32_code, pad):
    lib, (M, N, K) = ctx.lib, shape
    A, W, bias = _operands(M, N, K)
    Ab = _buf(A, K + pad)
    ldwt = (N + 31) // 32 * 32 + (32 if pad else 0)
    Wt = _buf(W.t().contiguous(), ldwt, NAN)  # the padding must never reach a result
    prod = _product(M, N, K, False)
    ws_bytes = int(lib.gdmcf_linear_ws_bytes(M, N, K))
    ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=DEV)
    C = torch.empty(M, N + pad, device=DEV)
    for act, use_bias in [(0, 1), (1, 1), (0, 0), (1, 0)]:
        what = ("fwd_wt", shape, pad, act, use_bias)

        def launch():
            C.fill_(NAN)
            _lib.check(lib.gdmcf_linear_fwd_wt_f32(Ab.data_ptr(), K + pad, Wt.data_ptr(), ldwt, bias.data_ptr() if use_bias else None,
                                                   act, M, N, K, C.data_ptr(), N + pad, ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (C.clone(),)

        code, (c,) = _twice(launch, what)
        _route("fwd_wt", ctx, shape, pad, code)
        assert code == f32_code, (what, code)
        ref = prod + bias.double() if use_bias else prod
        _close(c[:, :N], torch.tanh(ref) if act else ref, what)
        assert _all_nan(c[:, N:]), what + ("guard columns written",)


@pytest.mark.parametrize("shape,f32_code", WT_SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _ in WT_SHAPES])
def test_transposed_weight_forward(shape, f32_code):
    with _mode("f32") as ctx:
        _each_pad(ctx, _wt_case, shape, f32_code)


@pytest.mark.parametrize("mode", ["bf16", "f32x3"])
def test_transposed_weight_forward_refuses_other_modes(mode):
    M, N, K = 17, 33, 65
    with _mode(mode) as ctx:
        lib = ctx.lib
        A, W, bias = _operands(M, N, K)
        Wt = _buf(W.t().contiguous(), 64)
        ws_bytes = int(lib.gdmcf_linear_ws_bytes(M, N, K))
        ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=DEV)
        C = torch.full((M, N), NAN, device=DEV)
        rc = lib.gdmcf_linear_fwd_wt_f32(A.data_ptr(), K, Wt.data_ptr(), 64, bias.data_ptr(), 1, M, N, K, C.data_ptr(), N, ws.data_ptr(),
                                         ws_bytes, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.E_UNSUPPORTED
        assert _all_nan(C)
        assert "linear_fwd_wt" in lib.gdmcf_last_error().decode()


# ---- 4. optional arguments of the four common entries --------------------------------------------------------------------

# (M, N, K): family in f32 of forward / input gradient / weight gradient.  The input gradient is KC x MC over N (gemm_small when
# N < 4 or K < 4), the weight gradient MC x MC over M (gemm_small when N < 4 or K < 4; accumulate keeps the direct-to-register
# kernels away at any size); none of the shapes reaches a direct-to-register threshold.
OPT_SHAPES = [
    ((3, 2, 9), (1, 9, 9)),        # class 2; N < 4
    ((17, 33, 65), (1, 1, 1)),     # class 2; dW [33, 65]: class 2, a 1-column N tail in its second column tile
    ((81, 129, 33), (1, 1, 1)),    # forward class 1; dA [81, 33] class 2; dW [129, 33] class 2
    ((100, 257, 36), (1, 1, 1)),   # forward class 1; dW [257, 36] class 2
    ((129, 70, 4099), (1, 1, 1)),  # forward class 0, split over K; dA [129, 4099] class 0; dW [70, 4099] class 0, 3-column tail
]
OPT_CASES = [(m, s, c) for m in MODES for s, c in OPT_SHAPES]
OPT_IDS = [f"{m}-{s[0]}x{s[1]}x{s[2]}" for m, s, _ in OPT_CASES]


def _ws(lib, M, N, K):
    ws_bytes = int(lib.gdmcf_linear_ws_bytes(M, N, K))
    return torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device=DEV), ws_bytes


def _fwd_case(ctx, shape, codes, pad):
    lib, (M, N, K) = ctx.lib, shape
    A, lda, W, ldw, bias, out64 = _layer(ctx, M, N, K, pad)
    prod = _product(M, N, K, ctx.rounded)
    ws, ws_bytes = _ws(lib, M, N, K)
    C = torch.empty(M, N + pad, device=DEV)
    for act, use_bias in [(0, 1), (0, 0), (1, 0)]:
        what = ("fwd", ctx.mode, shape, pad, act, use_bias)

        def launch():
            C.fill_(NAN)
            _lib.check(lib.gdmcf_linear_fwd_f32(A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr() if use_bias else None, act, M, N, K,
                                                C.data_ptr(), N + pad, ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (C.clone(),)

        code, (c,) = _twice(launch, what)
        _route("fwd", ctx, shape, pad, code)
        assert code == ctx.code(codes[0]), (what, code)
        ref = out64 if use_bias else prod
        _close(c[:, :N], torch.tanh(ref) if act else ref, what)
        assert _all_nan(c[:, N:]), what + ("guard columns written",)


@pytest.mark.parametrize("mode,shape,codes", OPT_CASES, ids=OPT_IDS)
def test_forward_optional_arguments(mode, shape, codes):
    with _mode(mode) as ctx:
        _each_pad(ctx, _fwd_case, shape, codes)


def _loss_case(ctx, shape, codes, pad):
    lib, (M, N, K) = ctx.lib, shape
    A, lda, W, ldw, bias, out64 = _layer(ctx, M, N, K, pad)
    g = torch.Generator(device="cpu").manual_seed(13 + M + N)
    tgt = torch.randn(M, N, generator=g).to(DEV)
    alpha = (torch.rand(M, generator=g) + 0.5).to(DEV)
    tgtb = _buf(tgt, N + pad, NAN)
    diff = torch.empty(M, N + pad, device=DEV)
    out = torch.empty(M, N + pad, device=DEV)
    rowpart = torch.empty(M * lib.gdmcf_loss_tiles(N), device=DEV)
    rowsum = torch.empty(M + 1, device=DEV)
    got = {}
    for use_alpha, use_out in [(1, 1), (0, 1), (1, 0), (0, 0)]:
        what = ("loss", ctx.mode, shape, pad, use_alpha, use_out)

        def launch():
            for t in (diff, out, rowsum):
                t.fill_(NAN)
            rowpart.zero_()
            _lib.check(lib.gdmcf_linear_loss_fwd_f32(A.data_ptr(), lda, W.data_ptr(), ldw, bias.data_ptr(), tgtb.data_ptr(), N + pad,
                                                     alpha.data_ptr() if use_alpha else None, M, N, K,
                                                     out.data_ptr() if use_out else None, N + pad if use_out else 0, diff.data_ptr(),
                                                     N + pad, rowpart.data_ptr(), rowsum.data_ptr(), _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (diff.clone(), out.clone(), rowsum.clone())

        code, (d, o, rs) = _twice(launch, what)
        _route("loss", ctx, shape, pad, code)
        assert code == ctx.code(codes[0]), (what, code)
        dref = (alpha.double()[:, None] if use_alpha else 1.0) * out64 - tgt.double()
        _close(d[:, :N], dref, what + ("diff",))
        _close_rows(rs[:M], (dref * dref).sum(1), what + ("rowsum",))
        assert _all_nan(d[:, N:]) and _all_nan(rs[M:]), what + ("guard written",)
        if use_out:
            _close(o[:, :N], out64, what + ("out",))
            assert _all_nan(o[:, N:]), what + ("out guard columns written",)
        else:
            assert _all_nan(o), what + ("out written though NULL",)
            assert _same(d, got[(use_alpha, 1)][0]) and _same(rs, got[(use_alpha, 1)][1]), what + ("diff / rowsum differ without out",)
        got[(use_alpha, use_out)] = (d, rs)


@pytest.mark.parametrize("mode,shape,codes", OPT_CASES, ids=OPT_IDS)
def test_loss_optional_arguments(mode, shape, codes):
    with _mode(mode) as ctx:
        _each_pad(ctx, _loss_case, shape, codes)


@functools.lru_cache(maxsize=None)
def _grad_values(M, N, K):
    g = torch.Generator(device="cpu").manual_seed(17 + 41 * M + 43 * N + K)
    dZ = torch.randn(M, N, generator=g)
    rs = torch.rand(M, generator=g) + 0.5
    act = torch.rand(M, K, generator=g) * 1.8 - 0.9
    dW0 = torch.randn(N, K, generator=g)
    return dZ.to(DEV), rs.to(DEV), act.to(DEV), dW0.to(DEV)


def _bwd_input_case(ctx, shape, codes, pad):
    """dA = rowscale (dZ W) (1 - Aact^2), each factor optional"""
    lib, (M, N, K) = ctx.lib, shape
    _, W, _ = _operands(M, N, K)
    dZ, rs, act, _ = _grad_values(M, N, K)
    ldw = K + (1 if pad else 0)
    Wb, dZb, actb = _buf(W, ldw), _buf(dZ, N + pad), _buf(act, K + pad)
    ctx.operand_shadows(dZb[:, :N], Wb[:, :K])
    prod = _D(dZ, ctx.rounded) @ _D(W, ctx.rounded)
    ws, ws_bytes = _ws(lib, M, N, K)
    dA = torch.empty(M, K + pad, device=DEV)
    for use_rs, use_act in [(0, 1), (1, 0), (0, 0)]:
        what = ("bwd_input", ctx.mode, shape, pad, use_rs, use_act)

        def launch():
            dA.fill_(NAN)
            _lib.check(lib.gdmcf_linear_bwd_input_f32(dZb.data_ptr(), N + pad, Wb.data_ptr(), ldw, rs.data_ptr() if use_rs else None,
                                                      actb.data_ptr() if use_act else None, K + pad if use_act else 0, use_act, M, N, K,
                                                      dA.data_ptr(), K + pad, ws.data_ptr(), ws_bytes, _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (dA.clone(),)

        code, (d,) = _twice(launch, what)
        _route("bwd_input", ctx, shape, pad, code)
        assert code == ctx.code(codes[1]), (what, code)
        ref = prod
        if use_rs:
            ref = rs.double()[:, None] * ref
        if use_act:
            ref = ref * (1 - act.double() ** 2)
        _close(d[:, :K], ref, what)
        assert _all_nan(d[:, K:]), what + ("guard columns written",)


@pytest.mark.parametrize("mode,shape,codes", OPT_CASES, ids=OPT_IDS)
def test_input_gradient_optional_arguments(mode, shape, codes):
    with _mode(mode) as ctx:
        _each_pad(ctx, _bwd_input_case, shape, codes)


def _bwd_weight_case(ctx, shape, codes, pad):
    """dW = (dW0 +) dZ^T A, db = sum_m rowscale dZ"""
    lib, (M, N, K) = ctx.lib, shape
    A, _, _ = _operands(M, N, K)
    dZ, rs, _, dW0 = _grad_values(M, N, K)
    ldw = K + (1 if pad else 0)
    dZb = _buf(dZ, N + pad)
    Ab = _buf(A, K + pad)
    Acol = _buf(A, K + 8)   # column K holds rowscale
    Acol[:, K] = rs
    Aone = _buf(A, K + 8)   # column K holds 1
    Aone[:, K] = 1.0
    ctx.operand_shadows(dZb[:, :N], Ab[:, :K], Acol[:, :K], Aone[:, :K])
    prod = _D(dZ, ctx.rounded).t() @ _D(A, ctx.rounded)
    db_rs = (rs.double()[:, None] * dZ.double()).sum(0)
    db_plain = dZ.double().sum(0)
    dW = torch.empty(N, ldw, device=DEV)
    db = torch.empty(N + 1, device=DEV)
    # (operand, lda, rowscale, a_scale_col, db, accumulate)
    variants = [(Ab, K + pad, 1, 0, 1, 1), (Ab, K + pad, 1, 0, 0, 0), (Ab, K + pad, 0, 0, 1, 0), (Acol, K + 8, 1, 1, 1, 0),
                (Acol, K + 8, 1, 1, 1, 1)]
    if ctx.mode == "f32":
        variants.append((Aone, K + 8, 0, 1, 1, 0))
    for op, lda, use_rs, scale_col, use_db, accumulate in variants:
        what = ("bwd_weight", ctx.mode, shape, pad, "rowscale", use_rs, "a_scale_col", scale_col, "db", use_db, "accumulate", accumulate)

        def launch():
            dW.fill_(NAN)
            db.fill_(NAN)
            if accumulate:
                dW[:, :K] = dW0
            _lib.check(lib.gdmcf_linear_bwd_weight_f32(dZb.data_ptr(), N + pad, op.data_ptr(), lda, rs.data_ptr() if use_rs else None,
                                                       scale_col, M, N, K, dW.data_ptr(), ldw, db.data_ptr() if use_db else None,
                                                       accumulate, _lib.stream_ptr()))
            code = lib.gdmcf_debug_last_gemm()
            torch.cuda.synchronize()
            return code, (dW.clone(), db.clone())

        code, (w, b) = _twice(launch, what)
        _route("bwd_weight", ctx, shape, pad, code)
        assert code == ctx.code(codes[2]), (what, code)
        _close(w[:, :K], dW0.double() + prod if accumulate else prod, what + ("dW",))
        assert _all_nan(w[:, K:]), what + ("dW guard columns written",)
        if use_db:
            _close_db(b[:N], db_rs if use_rs else db_plain, what + ("db",))
            assert _all_nan(b[N:]), what + ("db guard written",)
        else:
            assert _all_nan(b), what + ("db written though NULL",)


@pytest.mark.parametrize("mode,shape,codes", OPT_CASES, ids=OPT_IDS)
def test_weight_gradient_optional_arguments(mode, shape, codes):
    with _mode(mode) as ctx:
        _each_pad(ctx, _bwd_weight_case, shape, codes)
