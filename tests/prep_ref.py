"""Host model of the denoiser-input builder (csrc/prep_input.hip), written from the contract of gdmcf_dnn_prep_input_f32 in
include/gdmcf_hip.h -- numpy only, no GPU, no gdmcf_amd import.  tests/test_host_prep.py checks the model itself (against the
oracle's timestep embedding and a float64 torch composition); tests/test_gpu_prep.py holds the dense builder, the two CSR builders
and gdmcf_dnn_emb_cols_f32 to it.

    xin[b, :] = [ drop( norm( ca[ts[b]] x[b, :] + cb[ts[b]] noise[b, :] ) ) | emb_b + emb_w @ temb(ts[b]) (E columns) | 1 | 0 ... ]

  xt32 / xin_items32        the float32 operations the contract names, one IEEE rounding each: held to equality
  rownorm64 / emb64         float64 references, with the bounds a float32 evaluation may leave them by (derived in the docstrings)
  temb64 / temb_scale       the sinusoids in float64 and the scale their float32 evaluation is measured in (TEMB_ERR_MEASURED)
  row64                     the whole row in float64 (the layout, and what test_host_prep.py compares with torch)
  pack_bits / bf16_bits     bits_out and the bf16 shadow
"""
import math

import numpy as np

from tests.glue_ref import F32, F64, U, row_norms_depth

# The one number that cannot be derived: how far the device's expf / sinf / cosf leave temb_out from temb64, in units of
# temb_scale.  Largest value over all 356 launches of tests/test_gpu_prep.py (every (I, E, ldxin) and mode of the four entries,
# ts = 0, 1, 999), measured on an MI355X on 2026-10-21 -- at E = 256, t = 999; the bound asserted everywhere is 4x that (libm
# error varies with the argument range).
TEMB_ERR_MEASURED = 0.8163
TEMB_TOL = 4 * TEMB_ERR_MEASURED
assert TEMB_TOL <= 64


def ceil4(n):
    return (n + 3) // 4 * 4


# ---- q_sample, F.normalize, dropout ---------------------------------------------------------------------------------------------
def xt32(x, ca=None, cb=None, noise=None):
    """x_t = fl(fl(ca x) + fl(cb n)) in float32 (ca, cb: float32 [B], already gathered at ts; noise None: zeros).  ca None: x."""
    x = np.asarray(x, dtype=F32)
    if ca is None:
        return x
    n = np.zeros_like(x) if noise is None else np.asarray(noise, dtype=F32)
    p0 = np.asarray(ca, dtype=F32)[:, None] * x
    p1 = np.asarray(cb, dtype=F32)[:, None] * n
    out = p0 + p1
    assert out.dtype == F32
    return out


def xt_draw_bound(x, ca, cb, normals64, normal_tol):
    """x_t with in-kernel normals: each normal is within normal_tol of the float64 model, which reaches x_t as normal_tol |cb|;
    the two products and the sum round once each, u (|ca x| + |cb n| + |x_t|) <= 2u (|ca x| + |cb n|) in all."""
    a = np.abs(np.asarray(ca, dtype=F64)[:, None] * np.asarray(x, dtype=F64))
    b = np.abs(np.asarray(cb, dtype=F64)[:, None] * normals64)
    return normal_tol * np.abs(np.asarray(cb, dtype=F64))[:, None] + 2.0 * U * (a + b)


def rownorm64(xt):
    """float64 L2 norms [B] of the float32 rows."""
    return np.sqrt((np.asarray(xt, dtype=F32).astype(F64) ** 2).sum(1))


def rownorm_rel_bound(cols):
    """prep_rowss_kernel adds a row's squares in d = 4 ceil(I / 1024) + 9 steps at most: a thread takes four columns per
    1024-column trip, one addition each, then six shuffle additions and three across the waves (glue_ref.row_norms_depth counts
    the same chain).  Every term is a square, so nothing cancels: the sum is off by at most (d + 1) u relative (d additions and
    the square's own rounding -- none when the compiler contracts it into an fma), the square root halves that and adds its own
    rounding: (d + 1) / 2 + 1 <= d / 2 + 2 units, the half unit to spare covering the second-order terms."""
    return (row_norms_depth(cols) / 2.0 + 2.0) * U


def drop_scale32(p):
    """fl(1 / fl(1 - p)) from the float32 p the entry receives"""
    return F32(1.0) / (F32(1.0) - F32(p))


def xin_items32(xt, rn=None, keep=None, p=0.0):
    """The item columns in float32: fl(fl(x_t / max(rn, 1e-12)) scale), 0 where dropped.  rn: the float32 norms the kernel left in
    rownorm_ws (None: no normalize); keep: bool [B, I] (None: drop_mode 0 -- no scaling at all)."""
    v = np.asarray(xt, dtype=F32)
    if rn is not None:
        v = v / np.maximum(np.asarray(rn, dtype=F32), F32(1e-12))[:, None]
    if keep is not None:
        v = np.where(keep, v * drop_scale32(p), F32(0.0))
    assert v.dtype == F32
    return v


# ---- timestep embedding -----------------------------------------------------------------------------------------------------
def _freqs(E):
    half = E // 2
    return np.exp(-math.log(10000.0) * np.arange(half, dtype=F64) / max(half, 1))


def temb64(ts, E):
    """[B, E] float64: [cos(t f_j), sin(t f_j), (0 if E odd)], f_j = exp(-ln(10000) j / half), half = E // 2."""
    t = np.asarray(ts, dtype=F64)[:, None]
    f = _freqs(E)[None, :]
    out = np.zeros((t.shape[0], E), dtype=F64)
    half = E // 2
    out[:, :half] = np.cos(t * f)
    out[:, half:2 * half] = np.sin(t * f)
    return out


def temb_scale(ts, E):
    """[B, E]: u (1 + t f_j (1 + |ln f_j|)) -- the unit temb_out's error is measured in.  The result's own rounding is the 1; the
    argument t f_j carries the float32 roundings of f_j (its exponent ln f_j is rounded before expf sees it: |ln f_j| u absolute,
    which is relative on f_j) and of the product, and d cos / d arg <= 1."""
    t = np.asarray(ts, dtype=F64)[:, None]
    f = _freqs(E)
    s = U * (1.0 + t * (f * (1.0 + np.abs(np.log(f))))[None, :])
    out = np.full((t.shape[0], E), U, dtype=F64)
    half = E // 2
    out[:, :half] = s
    out[:, half:2 * half] = s
    return out


def emb64(emb_w, emb_b, temb):
    """[B, E] float64: emb_b + emb_w @ temb, on the temb given (the kernel's own temb_out in the GPU tests)."""
    return np.asarray(emb_b, dtype=F64)[None, :] + np.asarray(temb, dtype=F64) @ np.asarray(emb_w, dtype=F64).T


def emb_bound(emb_w, emb_b, temb):
    """(E + 2) u (|emb_b| + |emb_w| @ |temb|): the kernel adds E products onto emb_b one after the other; a partial sum is bounded
    by the sum of the absolute terms and each step rounds once (the product too, unless contracted): E + 1 at most on any term,
    one to spare."""
    E = np.asarray(emb_b).shape[0]
    mag = np.abs(np.asarray(emb_b, dtype=F64))[None, :] + np.abs(np.asarray(temb, dtype=F64)) @ np.abs(np.asarray(emb_w, dtype=F64)).T
    return (E + 2) * U * mag


# ---- the whole row ----------------------------------------------------------------------------------------------------------------
def tail_columns(emb, I, ldxin, one=True):
    """[B, ldxin - I]: what follows the item columns -- the E embedding columns, 1 in column I + E when there is one (`one`:
    gdmcf_dnn_emb_cols_f32 writes none), zeros up to ldxin."""
    emb = np.asarray(emb)
    B, E = emb.shape
    out = np.zeros((B, ldxin - I), dtype=emb.dtype)
    out[:, :E] = emb
    if one and I + E < ldxin:
        out[:, E] = 1.0
    return out


def row64(x, ts, ldxin, ca=None, cb=None, noise=None, normalize=False, keep=None, p=0.0, emb_w=None, emb_b=None, E=0):
    """The contract in float64, [B, ldxin]: ca / cb are the tables (gathered at ts here)."""
    x = np.asarray(x, dtype=F64)
    B, I = x.shape
    xt = x
    if ca is not None:
        n = np.zeros_like(x) if noise is None else np.asarray(noise, dtype=F64)
        xt = np.asarray(ca, dtype=F64)[ts][:, None] * x + np.asarray(cb, dtype=F64)[ts][:, None] * n
    v = xt
    if normalize:
        v = xt / np.maximum(np.sqrt((xt ** 2).sum(1)), 1e-12)[:, None]
    if keep is not None:
        v = np.where(keep, v * (1.0 / (1.0 - float(F32(p)))), 0.0)
    emb = emb64(emb_w, emb_b, temb64(ts, E)) if E else np.zeros((B, 0))
    return np.concatenate([v, tail_columns(emb, I, ldxin)], axis=1)


# ---- bits_out and the bf16 shadow ----------------------------------------------------------------------------------------------------
def pack_bits(dense, ldbits=None):
    """uint32 [B, ldbits] (ceil(I / 32) when None): bit c & 31 of word c >> 5 is set iff dense[b, c] != 0; bits >= I are zero."""
    d = np.asarray(dense) != 0
    B, I = d.shape
    nw = (I + 31) // 32
    ldbits = nw if ldbits is None else ldbits
    assert ldbits >= nw
    padded = np.zeros((B, ldbits * 32), dtype=np.uint64)
    padded[:, :I] = d
    w = (padded.reshape(B, ldbits, 32) << np.arange(32, dtype=np.uint64)).sum(2)
    return w.astype(np.uint32)


def bf16_bits(a):
    """uint16: the bfloat16 nearest to each float32 (ties to even) -- add 0x7FFF plus the kept part's last bit, drop 16 bits.
    (Finite inputs: a NaN is not what the builder writes.)"""
    b = np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


# ---- the cases both prep modules walk through ---------------------------------------------------------------------------------------
# 4085: I + E = 4095, the 1 is the span's last column; 4086: the 1 is the next workgroup's first; 4090: the embedding straddles
# the span.  (1024, 8186, 8192 and 12290 repeat these edges one and two spans further on.)
WIDTHS_E10 = (1, 3, 4, 5, 1023, 1024, 1025, 4085, 4086, 4090, 4093, 4095, 4096, 4097, 8186, 8191, 8192, 8193, 12290)
EMB_SIZES = (0, 1, 2, 7, 10, 256, 257)
EMB_WIDTHS = (5, 4090, 4096)


def shape_table():
    """[(I, E, ldxin)]: every width at E = 10 and every embedding size at I = 5, 4090, 4096, each with ldxin = ceil4(I + E) + 4,
    with ldxin = I + E where that is a multiple of 4 (no 1 column, the canary right behind), and once with at least 64 columns
    of padding (the padding reaches into a further thread group)."""
    pairs = [(I, 10) for I in WIDTHS_E10] + [(I, E) for I in EMB_WIDTHS for E in EMB_SIZES if E != 10]
    out = []
    for I, E in pairs:
        out.append((I, E, ceil4(I + E) + 4))
        if (I + E) % 4 == 0:
            out.append((I, E, I + E))
    out.append((4090, 10, ceil4(4090 + 10 + 64)))
    return out
