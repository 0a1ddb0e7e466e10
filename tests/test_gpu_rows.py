"""GPU (-m gpu): the row-wise kernels of csrc/rows.hip and gdmcf_rowscale_f32 (csrc/reduce.hip), each called through the C ABI
with raw pointers and leading dimensions and compared with a CPU reference of tests/glue_ref.py: bit for bit where the kernel does
one float32 operation per element (densify_rows, gather_rows, scatter_add_rows, rowscale, scale), inside a bound derived from the
float64 reference's own terms where it sums (tanh_bwd, row_norms, normalize_rows_bwd, emb_bwd).  Outputs start as NaN, everything
between and behind the rows as a canary that must survive; inputs come from seeded CPU generators."""
import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(rc):
    _lib.check(rc)
    torch.cuda.synchronize()


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _f64(t):
    return t.detach().cpu().double().numpy()


# ---- bit-exact entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("I", [1, 3, 4, 5, 1023, 1024, 1030, 2051])
def test_densify_rows(I, pad):
    """Seven rows against a numpy scatter into zeros: ldo = I (rows alternately 16-byte aligned and not when I is odd: both zero
    fills) and I + 3, row_ids NULL / descending with a repeat, values NULL / random, an empty and a full row, columns -1, I and
    I + 5 that write nothing."""
    lib = _lib.load()
    indptr, indices = R.csr_case(I, seed=3)
    vals = np.random.default_rng(I).standard_normal(len(indices)).astype(np.float32)
    B, ldo = len(R.ROW_IDS), I + pad
    d_ip, d_ix, d_v, d_ids = _dev(indptr), _dev(indices), _dev(vals), _dev(np.array(R.ROW_IDS, dtype=np.int64))
    for ids in (None, R.ROW_IDS):
        for values in (None, vals):
            buf, out = R.seat(B, I, ldo, DEV)
            _run(lib.gdmcf_densify_rows_f32(d_ip.data_ptr(), d_ix.data_ptr(), None if values is None else d_v.data_ptr(),
                                            None if ids is None else d_ids.data_ptr(), B, I, out.data_ptr(), ldo,
                                            _lib.stream_ptr()))
            want = R.densify(indptr, indices, values, ids, B, I)
            assert np.array_equal(out.cpu().numpy(), want), (ids is None, values is None)
            assert R.canary_intact(buf, B, I, ldo)


@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("cols", [1, 255, 256, 257, 1000])
def test_gather_rows_and_scatter_add_rows(cols, n):
    """Distinct ids (one add per element: the sum is dst.index_add's, bit for bit), both strides wider than the rows, rows of dst
    that no id names unchanged."""
    lib = _lib.load()
    rows, lds, ldd = 131, cols + 5, cols + 3
    g = torch.Generator().manual_seed(cols * 131 + n)
    index = torch.randperm(rows, generator=g)[:n].contiguous()
    d_index = index.to(DEV)
    # gather: dst[j, :] = table[index[j], :]
    table = torch.randn(rows, cols, generator=g)
    tbuf, tview = R.seat(rows, cols, lds, DEV, table)
    obuf, out = R.seat(n, cols, ldd, DEV)
    _run(lib.gdmcf_gather_rows_f32(tview.data_ptr(), lds, d_index.data_ptr(), n, cols, out.data_ptr(), ldd, _lib.stream_ptr()))
    assert torch.equal(out.cpu(), table[index]) and R.canary_intact(obuf, n, cols, ldd)
    assert torch.equal(tview.cpu(), table) and R.canary_intact(tbuf, rows, cols, lds)
    # scatter-add: dst[index[j], :] += src[j, :]
    src, dst0 = torch.randn(n, cols, generator=g), torch.randn(rows, cols, generator=g)
    sbuf, sview = R.seat(n, cols, lds, DEV, src)
    dbuf, dst = R.seat(rows, cols, ldd, DEV, dst0)
    _run(lib.gdmcf_scatter_add_rows_f32(sview.data_ptr(), lds, d_index.data_ptr(), n, cols, dst.data_ptr(), ldd,
                                        _lib.stream_ptr()))
    got = dst.cpu()
    assert torch.equal(got, dst0.index_add(0, index, src)) and R.canary_intact(dbuf, rows, cols, ldd)
    others = torch.ones(rows, dtype=torch.bool)
    others[index] = False
    assert int(others.sum()) == rows - n and torch.equal(got[others], dst0[others])
    assert not torch.equal(got[index], dst0[index])


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 4, 5, 1023, 1024, 1025, 2050])
def test_rowscale(K, M):
    """out = A * rs[:, None] in float32, lda odd.  ldo = K: nothing behind the row; ldo = K + 3: column K holds rs, the two
    columns behind it stay."""
    lib = _lib.load()
    rng = np.random.default_rng(K * 7 + M)
    A, rs = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal(M).astype(np.float32)
    lda = K + 2 if K % 2 else K + 1
    abuf, a = R.seat(M, K, lda, DEV, A)
    d_rs = _dev(rs)
    for ldo in (K, K + 3):
        width = K if ldo == K else K + 1
        buf, out = R.seat(M, width, ldo, DEV)
        _run(lib.gdmcf_rowscale_f32(a.data_ptr(), lda, d_rs.data_ptr(), M, K, out.data_ptr(), ldo, _lib.stream_ptr()))
        got = out.cpu().numpy()
        assert np.array_equal(got[:, :K], A * rs[:, None])
        if ldo > K:
            assert np.array_equal(got[:, K], rs)
        assert R.canary_intact(buf, M, width, ldo)
    assert R.canary_intact(abuf, M, K, lda) and np.array_equal(a.cpu().numpy(), A)  # the input and its padding are as before


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_scale(n):
    lib = _lib.load()
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32)
    buf, out = R.seat(1, n, n, DEV)
    _run(lib.gdmcf_scale_f32(_dev(x).data_ptr(), n, 0.3, out.data_ptr(), _lib.stream_ptr()))
    assert np.array_equal(out.cpu().numpy()[0], x * np.float32(0.3)) and R.canary_intact(buf, 1, n, n)


# ---- entries held to a derived float32 bound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 9])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_tanh_bwd(N, M):
    """out = (dA + scale[0] * extra) * (1 - A^2) within 4u (|dA| + |scale extra|), |A| up to 0.9999, four distinct strides, with
    and without the addend."""
    lib = _lib.load()
    rng = np.random.default_rng(N * 11 + M)
    dA, extra = (rng.standard_normal((M, N)).astype(np.float32) for _ in range(2))
    A = rng.uniform(-0.9999, 0.9999, (M, N)).astype(np.float32)
    A.flat[::7] = np.float32(0.9999)
    A.flat[3::7] = np.float32(-0.9999)
    scale = np.float32(0.37)
    ldd, lda, lde, ldo = N + 1, N + 2, N + 3, N + 4
    _, d_dA = R.seat(M, N, ldd, DEV, dA)
    _, d_A = R.seat(M, N, lda, DEV, A)
    _, d_extra = R.seat(M, N, lde, DEV, extra)
    d_scale = _dev(np.array([scale]))
    for with_extra in (False, True):
        buf, out = R.seat(M, N, ldo, DEV)
        _run(lib.gdmcf_tanh_bwd_f32(d_dA.data_ptr(), ldd, d_A.data_ptr(), lda, d_extra.data_ptr() if with_extra else None, lde,
                                    d_scale.data_ptr() if with_extra else None, M, N, out.data_ptr(), ldo, _lib.stream_ptr()))
        want = R.tanh_bwd_ref(dA, A, extra if with_extra else None, float(scale))
        bound = R.tanh_bwd_bound(dA, extra if with_extra else None, float(scale))
        assert (np.abs(_f64(out) - want) <= bound).all(), with_extra
        assert R.canary_intact(buf, M, N, ldo)


def _needles(cols, *more):
    """The distinct columns among cols - 1, 0 and `more` that lie inside the row."""
    return sorted({c for c in (cols - 1, 0) + more if 0 <= c < cols})


@pytest.mark.parametrize("cols", [1, 3, 4, 5, 1023, 1024, 1025, 4099])
def test_row_norms(cols):
    """Five random rows inside (d / 2 + 2) u relative (1 / norm one u more) with d = 4 ceil(cols / 1024) + 9, ld odd, norm only /
    inverse only / both.  Needle rows -- zero but for a single 1.0 in the last column, the first tail column, column 1024 or
    column 0 -- must give exactly 1: a skipped element gives 0."""
    lib = _lib.load()
    rng = np.random.default_rng(cols)
    needles = _needles(cols, cols - cols % 4, 1024)
    rows = 5 + len(needles)
    X = rng.standard_normal((rows, cols)).astype(np.float32)
    X[5:] = 0.0
    for r, c in enumerate(needles):
        X[5 + r, c] = 1.0
    ld = cols + 2 if cols % 2 else cols + 1
    _, x = R.seat(rows, cols, ld, DEV, X)
    ref = np.sqrt((X.astype(np.float64) ** 2).sum(1))
    for want_norm, want_inv in ((True, False), (False, True), (True, True)):
        nbuf, norm = R.seat(1, rows, rows, DEV)
        ibuf, inv = R.seat(1, rows, rows, DEV)
        _run(lib.gdmcf_row_norms_f32(x.data_ptr(), ld, rows, cols, norm.data_ptr() if want_norm else None,
                                     inv.data_ptr() if want_inv else None, _lib.stream_ptr()))
        if want_norm:
            got = _f64(norm)[0]
            assert (np.abs(got - ref) <= R.row_norms_rel_bound(cols) * ref).all()
            assert (got[5:] == 1.0).all(), needles
        else:
            assert bool(torch.isnan(norm).all())
        if want_inv:
            got = _f64(inv)[0]
            assert (np.abs(got - 1.0 / ref) <= R.row_norms_rel_bound(cols, inverse=True) / ref).all()
            assert (got[5:] == 1.0).all(), needles
        else:
            assert bool(torch.isnan(inv).all())
        assert R.canary_intact(nbuf, 1, rows, rows) and R.canary_intact(ibuf, 1, rows, rows)


@pytest.mark.parametrize("cols", [4, 8, 1024, 1028, 4096, 1, 97, 4097, 4100, 5000])
def test_normalize_rows_bwd(cols):
    """dX = (dY - Y <dY, Y>) * inv_norm inside the derived bound on both branches (registers: cols <= 4096 and a multiple of 4;
    two passes otherwise), three distinct strides; once into a buffer of its own and once in place (dX == dY), bit-identical.  In
    the needle rows dY * Y is nonzero in one column only -- the last one, column 4096, the first column of the last group of a
    thread's walk -- so a dropped term moves the dot product by its whole value."""
    lib = _lib.load()
    rng = np.random.default_rng(cols)
    step = 1024 if (cols <= 4096 and cols % 4 == 0) else 256
    needles = _needles(cols, 4096, (cols - 1) // step * step)
    rows = 3 + len(needles)
    Xn = rng.standard_normal((rows, cols))
    norm = np.sqrt((Xn ** 2).sum(1))
    Y = (Xn / norm[:, None]).astype(np.float32)
    rn = (1.0 / norm).astype(np.float32)
    dY = rng.standard_normal((rows, cols)).astype(np.float32)
    dY[3:] = 0.0
    for r, c in enumerate(needles):
        dY[3 + r, c], Y[3 + r, c] = 1.0, 0.5
    lddy, ldy, lddx = cols + 1, cols + 2, cols + 3
    _, d_Y = R.seat(rows, cols, ldy, DEV, Y)
    d_rn = _dev(rn)
    want, bound = R.normalize_bwd_ref(dY, Y, rn), R.normalize_bwd_bound(dY, Y, rn)
    # into its own buffer
    ybuf, d_dY = R.seat(rows, cols, lddy, DEV, dY)
    buf, dX = R.seat(rows, cols, lddx, DEV)
    _run(lib.gdmcf_normalize_rows_bwd_f32(d_dY.data_ptr(), lddy, d_Y.data_ptr(), ldy, d_rn.data_ptr(), rows, cols, dX.data_ptr(),
                                          lddx, _lib.stream_ptr()))
    separate = dX.cpu()
    assert (np.abs(_f64(separate) - want) <= bound).all()
    assert R.canary_intact(buf, rows, cols, lddx) and np.array_equal(d_dY.cpu().numpy(), dY)
    # in place
    _run(lib.gdmcf_normalize_rows_bwd_f32(d_dY.data_ptr(), lddy, d_Y.data_ptr(), ldy, d_rn.data_ptr(), rows, cols,
                                          d_dY.data_ptr(), lddy, _lib.stream_ptr()))
    assert torch.equal(d_dY.cpu(), separate) and R.canary_intact(ybuf, rows, cols, lddy)


@pytest.mark.parametrize("I", [0, 37])
@pytest.mark.parametrize("E", [1, 3, 5, 10])
def test_emb_bwd(E, I):
    """demb = dZ1[:, :N] W1[:, I:I+E], dWe = demb^T temb, dbe = sum_m demb against float64 inside (ceil(N / 64) + ceil(M / 64) + 16) u
    times the same products of absolute values, N and M either side of the 64 lanes, lddz > N, ldw > I + E; workspace and
    results start as NaN (the entry overwrites, it does not accumulate)."""
    lib = _lib.load()
    rng = np.random.default_rng(E * 100 + I)
    for N in (1, 63, 64, 65, 200):
        for M in (1, 63, 65, 130):
            lddz, ldw = N + 3, I + E + 2
            dZ = rng.standard_normal((M, N)).astype(np.float32)
            W1 = rng.standard_normal((N, I + E)).astype(np.float32)
            temb = rng.standard_normal((M, E)).astype(np.float32)
            _, d_dZ = R.seat(M, N, lddz, DEV, dZ)
            _, d_W1 = R.seat(N, I + E, ldw, DEV, W1)
            d_temb = _dev(temb)
            wbuf, ws = R.seat(1, (M + N) * E, (M + N) * E, DEV)
            ebuf, dWe = R.seat(1, E * E, E * E, DEV)
            bbuf, dbe = R.seat(1, E, E, DEV)
            _run(lib.gdmcf_emb_bwd_f32(d_dZ.data_ptr(), lddz, d_W1.data_ptr(), ldw, I, E, d_temb.data_ptr(), M, N, ws.data_ptr(),
                                       dWe.data_ptr(), dbe.data_ptr(), _lib.stream_ptr()))
            want = R.emb_bwd_ref(dZ, W1, I, E, temb, N)
            bounds = R.emb_bwd_bounds(dZ, W1, I, E, temb, N)
            got = (_f64(ws)[0, :M * E].reshape(M, E), _f64(dWe).reshape(E, E), _f64(dbe)[0])
            for name, g, w, b in zip(("demb", "dWe", "dbe"), got, want, bounds):
                assert (np.abs(g - w) <= b).all(), (name, N, M)
            assert np.array_equal(ws.cpu().numpy()[0, M * E:].reshape(N, E), W1[:, I:])  # the gathered weight columns
            assert R.canary_intact(wbuf, 1, (M + N) * E, (M + N) * E) and R.canary_intact(ebuf, 1, E * E, E * E)
            assert R.canary_intact(bbuf, 1, E, E)
