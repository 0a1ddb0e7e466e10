"""GPU (-m gpu): the input builder at kernel level against the host model of its contract (tests/prep_ref.py, itself checked by
tests/test_host_prep.py): gdmcf_dnn_prep_input_f32, gdmcf_dnn_emb_cols_f32, gdmcf_dnn_prep_input_csr_f32 and
gdmcf_onehot_prep_input_csr_f32 at every width where the 4096-column workgroup span, the rolled tail pass and the embedding
columns meet.  The float32 operations the contract names (q_sample, the division by the norm, the dropout scale) are held to
equality; sums and sinusoids to bounds derived (or, for the device's libm, measured) in prep_ref.  Every output sits in a
canary-filled buffer (glue_ref.seat), NaN where the kernel must write; the inputs have row strides that are no multiple of 4
and start 4 bytes past a 16-byte boundary."""
import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import draws_ref as D
from tests import glue_ref as G
from tests import prep_ref as P
from tests.test_gpu_draws import NORMAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15
F32, F64 = np.float32, np.float64

T = 1000
_AB = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, T))
CA, CB = np.sqrt(_AB).astype(F32), np.sqrt(1.0 - _AB).astype(F32)  # a 1000-entry q_sample table
TS3 = np.array([0, 1, 999], dtype=np.int64)  # sinusoid arguments from 0 to 999

WORST = {"temb": 0.0, "at": None, "cases": 0}  # largest |temb_out - temb64| / temb_scale seen in this run


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def odd_ld(width):
    """a row stride > width that is no multiple of 4"""
    ld = width + 1
    return ld if ld % 4 else ld + 1


def strided(data, pad):
    """An input [rows, width] at a row stride that is no multiple of 4, starting one element into its buffer (4-byte, not 16-byte
    aligned for float32); `pad` fills what the kernel must not read.  Returns (keep-alive buffer, view)."""
    t = torch.as_tensor(np.ascontiguousarray(data))
    rows, width = t.shape
    ld = odd_ld(width)
    buf = torch.full((1 + rows * ld + 8,), pad, dtype=t.dtype, device=DEV)
    view = buf[1:1 + rows * ld].view(rows, ld)[:, :width]
    view.copy_(t)
    return buf, view


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def st():
    return _lib.stream_ptr()


class Seat:
    """An output window [rows, width] of row stride ld inside a canary-filled buffer (glue_ref.seat)."""

    def __init__(self, rows, width, ld, offset, data=None, dtype=torch.float32):
        self.geom = (rows, width, ld, offset)
        self.buf, self.view = G.seat(rows, width, ld, DEV, data=data, dtype=dtype, offset=offset)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        rows, width, ld, offset = self.geom
        assert G.canary_intact(self.buf, rows, width, ld, offset), "a store outside the output window"
        return self.view.cpu().numpy()


def emb_params(E, rng):
    if E == 0:
        return None, None
    return rng.standard_normal((E, E)).astype(F32), rng.standard_normal(E).astype(F32)


# ---- what every entry leaves behind the item columns ------------------------------------------------------------------------------
def check_temb(temb, ts, E, where):
    """temb_out against the float64 sinusoids, in units of prep_ref.temb_scale; the largest value of the run is kept."""
    err = np.abs(temb.astype(F64) - P.temb64(ts, E)) / P.temb_scale(ts, E)
    worst = float(err.max())
    WORST["cases"] += 1
    if worst > WORST["temb"]:
        WORST["temb"], WORST["at"] = worst, where
    assert worst <= P.TEMB_TOL, (where, worst, np.unravel_index(err.argmax(), err.shape))


def check_tail(xin, temb, ts, I, E, emb_w, emb_b, where, one=True):
    """columns [I, ldxin): the embedding columns within emb_bound of the float64 product on the kernel's own temb_out, then the 1
    (when there is room for it and the entry writes one) and zeros, exactly."""
    ldxin = xin.shape[1]
    if E:
        check_temb(temb, ts, E, where)
        ref, bound = P.emb64(emb_w, emb_b, temb), P.emb_bound(emb_w, emb_b, temb)
        err = np.abs(xin[:, I:I + E].astype(F64) - ref)
        assert (err <= bound).all(), (where, float((err / bound).max()))
    want = P.tail_columns(np.zeros((xin.shape[0], E), dtype=F32), I, ldxin, one=one)[:, E:]
    np.testing.assert_array_equal(xin[:, I + E:], want, err_msg=f"{where}: the 1 / the zero padding")


# ---- the dense builder ----------------------------------------------------------------------------------------------------------
def dense_case(I, E, ldxin, noise_mode=1, drop_mode=1, normalize=1, p=0.25, use_ca=True, zero_row=False, offset=7, shadow=None):
    """One launch of gdmcf_dnn_prep_input_f32 and every assertion on what it leaves.  Returns (xin seat, inputs) for the callers
    that look further (the bf16 shadow)."""
    where = dict(I=I, E=E, ldxin=ldxin, noise=noise_mode, drop=drop_mode, norm=normalize, p=p, ca=use_ca)
    B, ts = 3, TS3
    rng = np.random.default_rng([I, E, noise_mode, drop_mode])
    x = rng.uniform(-1.0, 1.0, (B, I)).astype(F32)
    if zero_row:
        x[1] = 0.0
    noise = rng.standard_normal((B, I)).astype(F32)
    keep = rng.random((B, I)) < 1.0 - p
    emb_w, emb_b = emb_params(E, rng)
    xb, xv = strided(x, float("nan"))
    nb, nv = strided(noise, float("nan"))
    kb, kv = strided(keep.astype(np.uint8), 1)
    ca, cb, tsd = dev(CA), dev(CB), dev(ts)
    ew, eb = (dev(emb_w), dev(emb_b)) if E else (None, None)
    ldxt = odd_ld(I)
    xin, xt_s = Seat(B, ldxin, ldxin, 4), Seat(B, I, ldxt, 1)
    temb_s = Seat(B, E, E, 2) if E else None
    rn_s = Seat(1, B, B, 1) if normalize else None
    if shadow is not None:
        shadow(xin)
    _lib.check(_lib.load().gdmcf_dnn_prep_input_f32(
        xv.data_ptr(), xv.stride(0), tsd.data_ptr(), ptr(ca) if use_ca else None, ptr(cb) if use_ca else None, noise_mode,
        nv.data_ptr() if noise_mode == 1 else None, nv.stride(0) if noise_mode == 1 else 0, drop_mode,
        kv.data_ptr() if drop_mode == 1 else None, kv.stride(0) if drop_mode == 1 else 0, p, SEED, offset, normalize, ptr(ew),
        ptr(eb), E, B, I, xin.ptr(), ldxin, xt_s.ptr(), ldxt, temb_s.ptr() if E else None, rn_s.ptr() if normalize else None, st()))
    torch.cuda.synchronize()
    got, xt = xin.get(), xt_s.get()
    # x_t
    if not use_ca:
        np.testing.assert_array_equal(xt, x, err_msg=f"{where}: x_t with ca == NULL")
    elif noise_mode == 2:
        nz = D.normals(B, I, D.STREAM_NOISE, SEED, offset)
        ref = CA[ts].astype(F64)[:, None] * x + CB[ts].astype(F64)[:, None] * nz
        err, bound = np.abs(xt - ref), P.xt_draw_bound(x, CA[ts], CB[ts], nz, NORMAL_TOL)
        assert (err <= bound).all(), (where, float((err / bound).max()))
    else:
        np.testing.assert_array_equal(xt, P.xt32(x, CA[ts], CB[ts], noise if noise_mode == 1 else None), err_msg=f"{where}: x_t")
    # the norm
    rn = None
    if normalize:
        rn = rn_s.get()[0]
        ref = P.rownorm64(xt)
        assert (np.abs(rn - ref) <= P.rownorm_rel_bound(I) * ref).all(), (where, rn, ref)
        if zero_row and (noise_mode == 0 or not use_ca):
            assert rn[1] == 0.0
    # the item columns, from the kernel's own x_t and norm
    if drop_mode == 2:
        keep = D.keep_mask(B, I, p, SEED, offset)
    items = P.xin_items32(xt, rn, keep if drop_mode else None, p)
    np.testing.assert_array_equal(got[:, :I], items, err_msg=f"{where}: item columns")
    check_tail(got, temb_s.get() if E else None, ts, I, E, emb_w, emb_b, where)
    return xin, (emb_w, emb_b)


SHAPES = P.shape_table()


@pytest.mark.parametrize("I,E,ldxin", SHAPES)
def test_dense_builder_every_width_and_embedding_size(I, E, ldxin):
    """Explicit noise, explicit keep-mask, F.normalize: x_t, the norm, the item columns, temb_out, the embedding columns, the 1 and
    the padding at every (I, E, ldxin) of prep_ref.shape_table."""
    dense_case(I, E, ldxin)


@pytest.mark.parametrize("I", [5, 4090, 4097])
def test_dense_builder_every_mode(I):
    """noise_mode x drop_mode x normalize x p, with the q_sample table and with ca = cb = NULL; a row of zeros wherever no noise
    is added, so that under normalize max(norm, 1e-12) is what divides."""
    E, ldxin, n = 10, P.ceil4(I + 10) + 4, 0
    for use_ca in (True, False):
        for noise_mode in ((0, 1, 2) if use_ca else (0,)):
            for drop_mode in (0, 1, 2):
                for normalize in (0, 1):
                    for p in (0.0, 0.25, 0.5):
                        n += 1
                        dense_case(I, E, ldxin, noise_mode, drop_mode, normalize, p, use_ca, zero_row=True, offset=100 + n)


# ---- gdmcf_dnn_emb_cols_f32 -------------------------------------------------------------------------------------------------------
def emb_cols_case(I, E, ldxin, shadow=None):
    B, ts = 3, TS3
    where = dict(entry="emb_cols", I=I, E=E, ldxin=ldxin)
    rng = np.random.default_rng([I, E, 77])
    emb_w, emb_b = emb_params(E, rng)
    init = np.full((B, ldxin), np.nan, dtype=F32)
    init[:, :I] = 3.5 + (np.arange(I) % 251)[None, :] + np.arange(B)[:, None] * 0.25  # the item columns are somebody else's
    xin, temb_s = Seat(B, ldxin, ldxin, 4, data=init), Seat(B, E, E, 2)
    ew, eb, tsd = dev(emb_w), dev(emb_b), dev(ts)
    if shadow is not None:
        shadow(xin)
    _lib.check(_lib.load().gdmcf_dnn_emb_cols_f32(tsd.data_ptr(), ew.data_ptr(), eb.data_ptr(), E, B, I, xin.ptr(), ldxin,
                                                  temb_s.ptr(), st()))
    torch.cuda.synchronize()
    got = xin.get()
    np.testing.assert_array_equal(got[:, :I], init[:, :I], err_msg=f"{where}: item columns touched")
    check_tail(got, temb_s.get(), ts, I, E, emb_w, emb_b, where, one=False)
    return xin


@pytest.mark.parametrize("I,E,ldxin", [s for s in SHAPES if s[1] > 0])
def test_emb_cols_every_width_and_embedding_size(I, E, ldxin):
    """The item columns stay as they were; columns [I, ldxin) are the embedding columns, then zeros -- and no 1: the reverse
    loop's first layer adds its bias itself."""
    emb_cols_case(I, E, ldxin)


# ---- the bf16 shadow ----------------------------------------------------------------------------------------------------------------
MARK16 = 7.0  # what the shadow holds where a kernel has to write (exact in bfloat16)


class Shadow:
    def __init__(self, B, cols, ldxin):
        self.B, self.cols = B, cols
        self.ld16 = (cols + 63) // 64 * 64
        self.reach = min(ldxin, self.ld16)
        self.buf = torch.zeros(64, self.ld16, dtype=torch.bfloat16, device=DEV)
        self.buf[:B, :self.reach] = MARK16
        self.f32 = None

    def __call__(self, xin):
        self.f32 = xin.ptr()
        _lib.check(_lib.load().gdmcf_bf16_shadow_set(self.f32, self.buf.data_ptr(), self.B, self.cols, self.ld16))

    def clear(self):
        if self.f32 is not None:
            _lib.load().gdmcf_bf16_shadow_clear(self.f32)

    def bits(self):
        return self.buf.cpu().view(torch.int16).numpy().view(np.uint16)


@pytest.mark.parametrize("I", [4090, 4097])
@pytest.mark.parametrize("wide", [False, True])
def test_builders_keep_the_bf16_shadow(I, wide):
    """A registered shadow of xin equals the bfloat16 rounding (nearest even) of xin bit for bit in columns < I + E and holds 0
    from column I + E on -- the 1 is the float32 matrix's alone -- up to min(ldxin, ld16); nothing else of it is written.  Both
    entries; `wide`: ldxin beyond the shadow's row."""
    E, B = 10, 3
    ldxin = (I + E + 63) // 64 * 64 + 4 if wide else P.ceil4(I + E) + 4
    mark = int(P.bf16_bits(np.array([MARK16], dtype=F32))[0])
    sh = Shadow(B, I + E, ldxin)
    try:
        xin, _ = dense_case(I, E, ldxin, shadow=sh)
        got, s = xin.get(), sh.bits()
        np.testing.assert_array_equal(s[:B, :I + E], P.bf16_bits(got[:, :I + E]))
        assert (s[:B, I + E:] == 0).all() and (s[B:] == 0).all()
    finally:
        sh.clear()
    sh = Shadow(B, I + E, ldxin)
    try:
        xin = emb_cols_case(I, E, ldxin, shadow=sh)
        got, s = xin.get(), sh.bits()
        assert (s[:B, :I] == mark).all(), "emb_cols wrote the shadow's item columns"
        np.testing.assert_array_equal(s[:B, I:I + E], P.bf16_bits(got[:, I:I + E]))
        assert (s[:B, I + E:] == 0).all() and (s[B:] == 0).all()
    finally:
        sh.clear()
    assert _lib.shadow_info(xin.ptr()) is None


# ---- the CSR sources ------------------------------------------------------------------------------------------------------------
CSR_ROWS = np.array([8, 8, 6, 4, 2, 1], dtype=np.int64)  # descending, a repeat, gaps; 4: strangers only, 2: full, 1: empty
BITS_MARK = 0x5A5A5A5A


def csr_matrix(I, seed):
    """glue_ref.csr_case (strangers -1, I, I + 5 in rows 0, 4, 6, 8; row 1 empty, rows 2 and 6 full) with one index of row 8
    stored twice."""
    indptr, indices = G.csr_case(I, seed)
    rows = [indices[indptr[r]:indptr[r + 1]] for r in range(9)]
    rows[8] = np.concatenate([rows[8], rows[8][:1], rows[8][-2:-1]])
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


def bits_seat(B, I, extra):
    nw = (I + 31) // 32
    ldbits = nw + extra
    return Seat(B, ldbits, ldbits, 3, data=np.full((B, ldbits), BITS_MARK, dtype=np.int32), dtype=torch.int32), nw, ldbits


def check_bits(seat, dense, nw, where):
    """words < ceil(I / 32): the packed rows, no bit >= I set; the words behind, inside ldbits: zero or untouched."""
    w = seat.get().view(np.uint32)
    np.testing.assert_array_equal(w[:, :nw], P.pack_bits(dense), err_msg=f"{where}: bits_out")
    assert np.isin(w[:, nw:], (0, BITS_MARK)).all(), (where, "words past ceil(I/32)")


CSR_MODES = [  # (use_ca, noise_mode, drop_mode, p, extra words of ldbits)
    (True, 1, 1, 0.25, 0), (True, 0, 2, 0.5, 3), (True, 1, 0, 0.0, 3), (True, 0, 1, 0.5, 0), (False, 0, 2, 0.25, 3),
    (True, 1, 2, 0.25, 0)]


@pytest.mark.parametrize("I", [5, 4090, 4097, 8193])
def test_csr_builder_is_the_model_on_the_densified_rows(I):
    """gdmcf_dnn_prep_input_csr_f32: xin is the model's on densify(rows) -- x_t bit for bit through the item columns (p = 0 or
    kept entries), the tail as the dense entry's -- and bits_out the packed rows: an index outside [0, I) sets no bit, a
    duplicated one sets its bit once."""
    E, ldxin, B = 10, P.ceil4(I + 10) + 4, len(CSR_ROWS)
    indptr, indices = csr_matrix(I, 5)
    x = G.densify(indptr, indices, None, CSR_ROWS, B, I)
    assert x[3].sum() == 0 and x[4].sum() == I and x[5].sum() == 0 and 0 < x[0].sum() < I
    ts = np.tile(TS3, 2)
    ip, ix, rows, tsd, ca, cb = dev(indptr), dev(indices), dev(CSR_ROWS), dev(ts), dev(CA), dev(CB)
    for n, (use_ca, noise_mode, drop_mode, p, extra) in enumerate(CSR_MODES):
        where = dict(entry="csr", I=I, ca=use_ca, noise=noise_mode, drop=drop_mode, p=p, extra=extra)
        rng = np.random.default_rng([I, n])
        noise = rng.standard_normal((B, I)).astype(F32)
        keep = rng.random((B, I)) < 1.0 - p
        emb_w, emb_b = emb_params(E, rng)
        nb, nv = strided(noise, float("nan"))
        kb, kv = strided(keep.astype(np.uint8), 1)
        ew, eb = dev(emb_w), dev(emb_b)
        xin, temb_s = Seat(B, ldxin, ldxin, 4), Seat(B, E, E, 2)
        bits, nw, ldbits = bits_seat(B, I, extra)
        offset = 300 + n
        _lib.check(_lib.load().gdmcf_dnn_prep_input_csr_f32(
            ip.data_ptr(), ix.data_ptr(), rows.data_ptr(), tsd.data_ptr(), ptr(ca) if use_ca else None,
            ptr(cb) if use_ca else None, noise_mode, nv.data_ptr() if noise_mode == 1 else None,
            nv.stride(0) if noise_mode == 1 else 0, drop_mode, kv.data_ptr() if drop_mode == 1 else None,
            kv.stride(0) if drop_mode == 1 else 0, p, SEED, offset, ew.data_ptr(), eb.data_ptr(), E, B, I, xin.ptr(), ldxin,
            temb_s.ptr(), bits.ptr(), ldbits, st()))
        torch.cuda.synchronize()
        got = xin.get()
        xt = P.xt32(x, CA[ts], CB[ts], noise if noise_mode == 1 else None) if use_ca else x
        if drop_mode == 2:
            keep = D.keep_mask(B, I, p, SEED, offset)
        np.testing.assert_array_equal(got[:, :I], P.xin_items32(xt, None, keep if drop_mode else None, p), err_msg=str(where))
        check_tail(got, temb_s.get(), ts, I, E, emb_w, emb_b, where)
        check_bits(bits, x, nw, where)


@pytest.mark.parametrize("E", [7, 10])
@pytest.mark.parametrize("I", [5, 2045, 2049, 4097])
def test_onehot_csr_builder_is_the_model_on_the_one_hot_image(I, E):
    """gdmcf_onehot_prep_input_csr_f32 with given classes: the 2I image columns are exactly {0, scale} -- column 2i + c is kept
    iff c is item i's class, the given class equals it and the keep-mask (explicit, then the model's draws) keeps it -- and the
    columns behind, sampled_out and bits_out are as for the dense source."""
    B, I2 = len(CSR_ROWS), 2 * I
    ldxin = P.ceil4(I2 + E) + 4
    indptr, indices = csr_matrix(I, 6)
    c0 = G.densify(indptr, indices, None, CSR_ROWS, B, I) != 0
    ts = np.tile(TS3, 2)
    ip, ix, rows, tsd = dev(indptr), dev(indices), dev(CSR_ROWS), dev(ts)
    for n, (drop_mode, p, extra) in enumerate([(1, 0.25, 0), (2, 0.5, 3), (0, 0.0, 3)]):
        where = dict(entry="onehot_csr", I=I, E=E, drop=drop_mode, p=p, extra=extra)
        rng = np.random.default_rng([I, E, n])
        sampled = (rng.random((B, I)) < 0.5).astype(np.uint8)
        keep = rng.random((B, I2)) < 1.0 - p
        emb_w, emb_b = emb_params(E, rng)
        sb, sv = strided(sampled, 1)
        kb, kv = strided(keep.astype(np.uint8), 1)
        ew, eb = dev(emb_w), dev(emb_b)
        xin, temb_s = Seat(B, ldxin, ldxin, 4), Seat(B, E, E, 2)
        ldso = odd_ld(I)
        so = Seat(B, I, ldso, 1, data=np.full((B, I), 9, dtype=np.uint8), dtype=torch.uint8)
        bits, nw, ldbits = bits_seat(B, I, extra)
        offset = 400 + n
        _lib.check(_lib.load().gdmcf_onehot_prep_input_csr_f32(
            ip.data_ptr(), ix.data_ptr(), rows.data_ptr(), None, 0.3, sv.data_ptr(), sv.stride(0), SEED, 1, so.ptr(), ldso,
            tsd.data_ptr(), drop_mode, kv.data_ptr() if drop_mode == 1 else None, kv.stride(0) if drop_mode == 1 else 0, p,
            offset, ew.data_ptr(), eb.data_ptr(), E, B, I, xin.ptr(), ldxin, temb_s.ptr(), bits.ptr(), ldbits, st()))
        torch.cuda.synchronize()
        got = xin.get()
        img = np.zeros((B, I, 2), dtype=F32)
        img[..., 0] = ~c0 & (sampled == 0)
        img[..., 1] = c0 & (sampled == 1)
        if drop_mode == 2:
            keep = D.keep_mask(B, I2, p, SEED, offset)
        want = P.xin_items32(img.reshape(B, I2), None, keep if drop_mode else None, p)
        assert set(np.unique(want)) <= {0.0, float(P.drop_scale32(p)) if drop_mode else 1.0}
        np.testing.assert_array_equal(got[:, :I2], want, err_msg=str(where))
        check_tail(got, temb_s.get(), ts, I2, E, emb_w, emb_b, where)
        np.testing.assert_array_equal(so.get(), sampled, err_msg=f"{where}: sampled_out")
        check_bits(bits, c0, nw, where)


# ---- the measured constant ---------------------------------------------------------------------------------------------------------
def test_temb_worst_case_of_the_run():
    """Prints the largest |temb_out - temb64| in units of prep_ref.temb_scale over every case this run has been through (the
    embedding-column entry's table when it is run alone): the figure TEMB_ERR_MEASURED records.  Measured on an MI355X over the
    whole module (356 launches): 0.8163, at E = 256 and t = 999; asserted everywhere: 4x that, 3.2652."""
    if WORST["cases"] == 0:
        for I, E, ldxin in SHAPES:
            if E:
                emb_cols_case(I, E, ldxin)
    print(f"\ntemb_out: largest |kernel - float64 model| / temb_scale over {WORST['cases']} launches = {WORST['temb']:.4f} "
          f"at {WORST['at']} (TEMB_ERR_MEASURED {P.TEMB_ERR_MEASURED}, asserted {P.TEMB_TOL})")
    assert 0.0 < WORST["temb"] <= P.TEMB_TOL
