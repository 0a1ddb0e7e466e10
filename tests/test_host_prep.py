"""CPU (-m "not gpu"): the host model of the input builder (tests/prep_ref.py) where no kernel is involved -- against the oracle's
timestep embedding, against a float64 torch composition of q_sample, F.normalize, dropout and cat, its bitmap packer and bfloat16
rounding against torch, its bounds against a float32 evaluation of the same sums -- and the argument checks with which the
builder's entries refuse before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gdmcf_amd import _lib
from oracle import gdmcf_oracle as O
from tests import prep_ref as P

F32, F64, U = np.float32, np.float64, P.U
TS = np.array([0, 1, 7, 999], dtype=np.int64)


# ---- the model against torch -------------------------------------------------------------------------------------------------------
def test_temb64_of_a_single_column_is_zero():
    """E = 1: half = 0, no sinusoid, the odd column alone.  (torch's composition has nothing to take the zero column's shape from
    there and returns no column at all; the builder's row keeps its E columns.)"""
    assert np.array_equal(P.temb64(TS, 1), np.zeros((len(TS), 1)))
    assert np.array_equal(P.temb_scale(TS, 1), np.full((len(TS), 1), U))


@pytest.mark.parametrize("E", [2, 3, 7, 10, 256, 257])
def test_temb64_is_the_oracles_timestep_embedding(E):
    """The oracle evaluates the sinusoids in float32.  Its result rounds once (<= 1 ulp <= 2u for |cos| <= 1); its argument t f
    carries exp's own ulp (2u relative), the product's rounding (u) and three relative roundings of the exponent ln f (the float32
    of -ln 10000, the product with j, the division by half), each |ln f| u on f: 3u t f (1 + |ln f|) in all.  Together no more
    than 3 temb_scale."""
    want = O.timestep_embedding(torch.from_numpy(TS), E).numpy()
    got = P.temb64(TS, E)
    assert got.shape == want.shape == (len(TS), E)
    err = np.abs(got - want.astype(F64)) / P.temb_scale(TS, E)
    assert err.max() <= 3.0, float(err.max())
    if E % 2:
        assert (got[:, -1] == 0).all()
    if E >= 2:
        assert (got[0, :E // 2] == 1).all() and (got[0, E // 2:] == 0).all()  # t = 0


def _case(B, I, E, seed):
    rng = np.random.default_rng([seed, I, E])
    x = rng.uniform(-1, 1, (B, I)).astype(F32)
    noise = rng.standard_normal((B, I)).astype(F32)
    keep = rng.random((B, I)) < 0.6
    ca, cb = rng.uniform(0.1, 1, 1000).astype(F32), rng.uniform(0.1, 1, 1000).astype(F32)
    emb_w = rng.standard_normal((max(E, 1), max(E, 1))).astype(F32)[:E, :E]
    emb_b = rng.standard_normal(E).astype(F32)
    return x, noise, keep, ca, cb, emb_w, emb_b


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("I,E,ldxin", [(1, 0, 4), (5, 1, 12), (5, 7, 12), (6, 10, 16), (12, 10, 28), (13, 2, 16)])
def test_row64_is_torchs_composition(I, E, ldxin, normalize):
    """[ dropout(F.normalize(q_sample)) | emb_layer(timestep_embedding) | 1 | 0 ] composed with torch in float64; the 1 only
    when I + E < ldxin."""
    B, p = 4, 0.25
    x, noise, keep, ca, cb, emb_w, emb_b = _case(B, I, E, 1)
    got = P.row64(x, TS, ldxin, ca, cb, noise, normalize, keep, p, emb_w, emb_b, E)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))  # noqa: E731
    xt = t(ca)[TS][:, None] * t(x) + t(cb)[TS][:, None] * t(noise)
    v = F.normalize(xt, dim=1) if normalize else xt
    v = v * t(keep) / (1.0 - p)
    parts = [v]
    if E:
        parts.append(F.linear(t(P.temb64(TS, E)), t(emb_w), t(emb_b)))
    pad = torch.zeros(B, ldxin - I - E, dtype=torch.float64)
    if I + E < ldxin:
        pad[:, 0] = 1.0
    want = torch.cat(parts + [pad], dim=1).numpy()
    assert got.shape == (B, ldxin)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)  # (two float64 evaluations: summation order only)
    assert (got[:, I + E + 1:] == 0).all()
    if (I + E) == ldxin:
        assert got.shape[1] == I + E  # no room for the 1


def test_float32_operations_stay_within_their_roundings_of_row64():
    """xt32 and xin_items32 on the float32 of rownorm64: x_t rounds three times relative to |ca x| + |cb n| (2u of it, see
    xt_draw_bound), which the division and the scale carry along; the norm's float32, the division, the float32 scale and the
    product round once each (u / 2 apiece, 4u allowed) relative to the result."""
    B, I, p = 4, 37, 0.25
    x, noise, keep, ca, cb, _, _ = _case(B, I, 0, 2)
    xt = P.xt32(x, ca[TS], cb[TS], noise)
    rn = P.rownorm64(xt).astype(F32)
    got = P.xin_items32(xt, rn, keep, p)
    want = P.row64(x, TS, I, ca, cb, noise, True, keep, p)
    mag = np.abs(ca[TS].astype(F64)[:, None] * x) + np.abs(cb[TS].astype(F64)[:, None] * noise)
    # the norm itself moves by at most 2u |mag|_2 / |x_t|_2 relative: a factor on every element of the row
    norm_shift = 2.0 * U * np.sqrt((mag ** 2).sum(1)) / np.sqrt((xt.astype(F64) ** 2).sum(1))
    bound = 2.0 * U * mag / rn.astype(F64)[:, None] / (1 - p) + (4.0 * U + norm_shift)[:, None] * np.abs(want)
    assert (np.abs(got - want) <= bound).all()
    assert (got[~keep] == 0).all() and got.dtype == F32
    # ca == NULL: x itself; drop_mode 0: no scale; a row of zeros divides by 1e-12
    assert P.xt32(x) is not None and np.array_equal(P.xt32(x), x)
    z = np.zeros((1, 5), dtype=F32)
    assert np.array_equal(P.xin_items32(z, P.rownorm64(z).astype(F32)), z)
    assert np.array_equal(P.xin_items32(x, None, None, 0.5), x)
    assert P.drop_scale32(0.5) == 2.0 and P.drop_scale32(0.0) == 1.0


@pytest.mark.parametrize("I", [1, 5, 31, 32, 33, 64, 4097])
def test_pack_bits_against_torch(I):
    B = 3
    d = np.random.default_rng(I).random((B, I)) < 0.4
    d[:, -1] = True
    for ldbits in (None, (I + 31) // 32 + 3):
        got = P.pack_bits(d, ldbits)
        nw = got.shape[1]
        pad = torch.zeros(B, nw * 32, dtype=torch.int64)
        pad[:, :I] = torch.from_numpy(d)
        want = (pad.view(B, nw, 32) * (2 ** torch.arange(32, dtype=torch.int64))).sum(-1).numpy()
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got.astype(np.int64), want)
        unpacked = ((got[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, -1)
        assert (unpacked[:, I:] == 0).all() and np.array_equal(unpacked[:, :I] != 0, d)


def test_bf16_bits_against_torch():
    rng = np.random.default_rng(0)
    a = np.concatenate([
        rng.standard_normal(4096).astype(F32) * F32(10.0) ** rng.integers(-30, 30, 4096).astype(F32),
        np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, -(1.0 + 2.0 ** -8),
                  1e-40, 3.3e38, 3.4028235e38, 2.0 ** -126, 1.0 - 2.0 ** -9], dtype=F32)])
    want = torch.from_numpy(a).bfloat16().view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(P.bf16_bits(a), want)
    assert P.bf16_bits(np.array([1.0 + 2.0 ** -8], dtype=F32))[0] == 0x3F80  # the tie goes to the even neighbour
    assert P.bf16_bits(np.array([1.0 + 3 * 2.0 ** -8], dtype=F32))[0] == 0x3F82


# ---- the bounds against a float32 evaluation of the same sums --------------------------------------------------------------------------
def _rowss_f32(row):
    """The L2 norm in float32 in the order the contract's depth is read from: 256 partial sums, each over four consecutive columns
    per 1024-column trip; a butterfly over each 64; the four results added one after the other; one square root."""
    I = len(row)
    padded = np.zeros(-(-I // 1024) * 1024, dtype=F32)
    padded[:I] = row
    part = np.zeros(256, dtype=F32)
    for trip in padded.reshape(-1, 256, 4):
        for j in range(4):
            part = part + trip[:, j] * trip[:, j]
    part = part.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ o]
    s = part[:, 0]
    assert s.dtype == F32
    return np.sqrt(((s[0] + s[1]) + s[2]) + s[3])


@pytest.mark.parametrize("I", [1, 5, 1025, 4097, 8193])
def test_rownorm_bound_holds_for_a_float32_evaluation(I):
    assert P.rownorm_rel_bound(I) == ((4 * -(-I // 1024) + 9) / 2.0 + 2.0) * U
    rng = np.random.default_rng(I)
    for scale in (1.0, 1e-3):
        xt = (rng.standard_normal((3, I)) * scale).astype(F32)
        ref = P.rownorm64(xt)
        got = np.array([_rowss_f32(r) for r in xt])
        assert (np.abs(got - ref) <= P.rownorm_rel_bound(I) * ref).all()


@pytest.mark.parametrize("E", [1, 7, 10, 257])
def test_emb_bound_holds_for_a_float32_evaluation(E):
    rng = np.random.default_rng(E)
    emb_w, emb_b = rng.standard_normal((E, E)).astype(F32), rng.standard_normal(E).astype(F32)
    temb = P.temb64(TS, E).astype(F32)
    e = np.broadcast_to(emb_b, (len(TS), E)).copy()
    for f in range(E):  # E multiply-adds one after the other, product and sum rounded separately
        e = e + emb_w[None, :, f] * temb[:, f:f + 1]
    assert e.dtype == F32
    ref, bound = P.emb64(emb_w, emb_b, temb), P.emb_bound(emb_w, emb_b, temb)
    assert (np.abs(e - ref) <= bound).all()
    assert (bound <= (E + 2) * U * (np.abs(emb_b)[None] + np.abs(emb_w).sum(1)[None] + 1e-30)).all()  # |temb| <= 1


def test_tail_columns_and_the_shape_table():
    emb = np.arange(6, dtype=F64).reshape(2, 3) + 5
    t = P.tail_columns(emb, 4, 12)
    assert t.shape == (2, 8) and (t[:, :3] == emb).all() and (t[:, 3] == 1).all() and (t[:, 4:] == 0).all()
    assert (P.tail_columns(emb, 5, 8) == emb).all()  # ldxin == I + E: no 1
    assert (P.tail_columns(emb, 4, 12, one=False)[:, 3:] == 0).all()
    table = P.shape_table()
    assert len(set(table)) == len(table)
    for I, E, ldxin in table:
        assert ldxin % 4 == 0 and ldxin >= I + E
    for I in P.WIDTHS_E10:
        assert (I, 10, P.ceil4(I + 10) + 4) in table
    for I in P.EMB_WIDTHS:
        for E in P.EMB_SIZES:
            assert (I, E, P.ceil4(I + E) + 4) in table
    assert (4086, 10, 4096) in table and (4090, 10, 4100) in table and (4096, 256, 4352) in table  # ldxin == I + E
    assert any(ldxin >= I + E + 64 for I, E, ldxin in table)


# ---- the entries refuse before any launch ---------------------------------------------------------------------------------------------
# Non-null stand-ins for the pointer arguments: host memory the checks never dereference.  16-byte aligned, as xin must be.
_MEM = ctypes.create_string_buffer(4096 + 16)
PTR = (ctypes.addressof(_MEM) + 15) & ~15


def dense_args(**kw):
    """Valid arguments of gdmcf_dnn_prep_input_f32 for B = 2, I = 40, E = 10, then `kw` on top."""
    a = dict(x=PTR, ldx=40, ts=PTR, ca=PTR, cb=PTR, noise_mode=1, noise=PTR, ldn=40, drop_mode=1, keep=PTR, ldkeep=40, drop_p=0.5,
             seed=3, offset=2, normalize=1, emb_w=PTR, emb_b=PTR, E=10, B=2, I=40, xin=PTR, ldxin=52, xt_out=PTR, ldxt=41,
             temb_out=PTR, rownorm_ws=PTR, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def csr_args(**kw):
    """Valid arguments of gdmcf_dnn_prep_input_csr_f32 for B = 2, I = 40, E = 10, then `kw` on top."""
    a = dict(indptr=PTR, indices=PTR, rows=PTR, ts=PTR, ca=PTR, cb=PTR, noise_mode=1, noise=PTR, ldn=40, drop_mode=1, keep=PTR,
             ldkeep=40, drop_p=0.5, seed=3, offset=2, emb_w=PTR, emb_b=PTR, E=10, B=2, I=40, xin=PTR, ldxin=52, temb_out=PTR,
             bits_out=PTR, ldbits=2, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


def onehot_args(**kw):
    """Valid arguments of gdmcf_onehot_prep_input_csr_f32 for B = 2, I = 40 (80 image columns), E = 10, then `kw` on top."""
    a = dict(indptr=PTR, indices=PTR, rows=PTR, ts_U=None, discrete=0.3, sampled=PTR, lds=40, seed=3, offset_noise=1,
             sampled_out=PTR, ldso=40, ts=PTR, drop_mode=1, keep=PTR, ldkeep=80, drop_p=0.5, offset_prep=2, emb_w=PTR, emb_b=PTR,
             E=10, B=2, I=40, xin=PTR, ldxin=92, temb_out=PTR, bits_out=PTR, ldbits=2, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return list(a.values())


SHAPE_REFUSALS = (dict(ldxin=54), dict(ldxin=48), dict(xin=PTR + 4))  # ldxin % 4, ldxin < I + E, a misaligned xin
ARG_REFUSALS = (dict(noise=None), dict(drop_p=1.0), dict(ts=None), dict(noise_mode=3), dict(keep=None), dict(ca=None))


def test_dense_entry_refuses_before_launching():
    lib = _lib.load()
    f = lib.gdmcf_dnn_prep_input_f32
    for kw in SHAPE_REFUSALS + (dict(ldx=39), dict(B=0)):
        assert f(*dense_args(**kw)) == _lib.E_SHAPE, kw
    for kw in ARG_REFUSALS + (dict(rownorm_ws=None),):  # (normalize without its scratch)
        assert f(*dense_args(**kw)) == _lib.E_ARG, kw
    assert b"prep_input" in lib.gdmcf_last_error()
    assert f(*dense_args(ca=None, cb=None, noise_mode=0, noise=None, E=0, emb_w=None, emb_b=None, ts=None, rownorm_ws=None)) \
        == _lib.E_ARG  # every other argument is fine without ts, ca and the embedding: only the scratch is missing


def test_csr_entry_refuses_before_launching():
    lib = _lib.load()
    f = lib.gdmcf_dnn_prep_input_csr_f32
    for kw in SHAPE_REFUSALS + (dict(I=0),):
        assert f(*csr_args(**kw)) == _lib.E_SHAPE, kw
    for kw in ARG_REFUSALS + (dict(ldbits=1), dict(indptr=None), dict(rows=None)):  # ldbits < ceil(40 / 32)
        assert f(*csr_args(**kw)) == _lib.E_ARG, kw
    assert b"prep_input_csr" in lib.gdmcf_last_error()


def test_onehot_csr_entry_refuses_before_launching():
    lib = _lib.load()
    f = lib.gdmcf_onehot_prep_input_csr_f32
    for kw in (dict(ldxin=94), dict(ldxin=88), dict(xin=PTR + 4), dict(B=0)):  # ldxin % 4, ldxin < 2I + E, alignment
        assert f(*onehot_args(**kw)) == _lib.E_SHAPE, kw
    for kw in (dict(drop_p=1.0), dict(ts=None), dict(keep=None), dict(ldkeep=79), dict(ldbits=1), dict(lds=39),
               dict(sampled=None), dict(ldso=39)):
        assert f(*onehot_args(**kw)) == _lib.E_ARG, kw
    assert b"onehot_prep_input_csr" in lib.gdmcf_last_error()
