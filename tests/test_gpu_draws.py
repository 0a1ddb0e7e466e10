"""GPU (-m gpu): every in-kernel random draw against the host model of the documented contract (tests/draws_ref.py, pinned to
the Random123 vectors by tests/test_host_draws.py): integer and bit draws exactly, normals within NORMAL_TOL.  The draws are a
persisted format -- checkpoints store (seed, offset) and other kernels regenerate them -- so the contract, not another kernel,
is the reference here."""
import numpy as np
import pytest
import torch

import gdmcf_amd
from gdmcf_amd import ModelMeanType, _lib
from tests import draws_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x9E3779B97F4A7C15  # both key words in use
# Largest |gdmcf_randn_f32 - float64 model| measured over the cases of test_randn_matches_the_model on an MI355X; the bound
# asserted everywhere is 4x that (hardware log / sin / cos are not correctly rounded and their error depends on the input range).
NORMAL_ERR_MEASURED = 4.705e-7
NORMAL_TOL = 4 * NORMAL_ERR_MEASURED
assert NORMAL_TOL <= 1e-4


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def st():
    return _lib.stream_ptr()


def randn(rows, cols, ld, stream, seed, offset, fill=-7.0):
    out = torch.full((rows, ld), fill, dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().gdmcf_randn_f32(out.data_ptr(), ld, rows, cols, stream, seed, offset, st()))
    return out.cpu().numpy()


RANDN_SHAPES = [(3, 1, 4), (2, 5, 8), (3, 1027, 1032), (2, 4099, 4100)]


def test_randn_matches_the_model():
    """gdmcf_randn_f32 against the float64 Box-Muller of the contract: every (rows, cols, ld) x stream x offset.  Measured on an
    MI355X: largest absolute difference over the 24 cases 4.705e-07 (printed below on every run); asserted: 4x that, 1.882e-06."""
    worst = 0.0
    for rows, cols, ld in RANDN_SHAPES:
        for stream in (0, 4, 7):
            for offset in (1, 2 ** 32 - 1):
                got = randn(rows, cols, ld, stream, SEED, offset)
                assert (got[:, cols:] == -7.0).all(), "columns past `cols` were written"
                ref = R.normals(rows, cols, stream, SEED, offset)
                err = float(np.abs(got[:, :cols].astype(np.float64) - ref).max())
                worst = max(worst, err)
                assert err <= NORMAL_TOL, (rows, cols, ld, stream, offset, err)
    print(f"\nrandn: largest |kernel - float64 model| over {len(RANDN_SHAPES) * 6} cases = {worst:.3e} (NORMAL_TOL {NORMAL_TOL:.1e})")


# ---- the dense input builder: noise_mode 2, drop_mode 2 -----------------------------------------------------------------------
CA = np.array([1.0, 0.9, 0.75], dtype=np.float32)
CB = np.array([1.0, 0.5, 0.25], dtype=np.float32)  # powers of two: cb * normal is exact in float32


def _builder(x, ts, p, E, offset, seed=SEED):
    """gdmcf_dnn_prep_input_f32 with in-kernel noise and dropout; returns (xin [B, ldxin], xt [B, I]) as numpy."""
    B, I = x.shape
    ldxin = (I + E + 3) // 4 * 4 + 4  # > I + E
    xin = torch.full((B, ldxin), -3.0, dtype=torch.float32, device=DEV)
    xt = torch.full((B, I + 3), -3.0, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(E)
    emb_w = torch.randn(max(E, 1), max(E, 1), generator=g).to(DEV)
    emb_b = torch.randn(max(E, 1), generator=g).to(DEV)
    temb = torch.zeros(B, max(E, 1), device=DEV)
    xd, tsd, ca, cb = dev(x), dev(ts), dev(CA), dev(CB)
    _lib.check(_lib.load().gdmcf_dnn_prep_input_f32(
        xd.data_ptr(), xd.stride(0), tsd.data_ptr(), ca.data_ptr(), cb.data_ptr(), 2, None, 0, 2, None, 0, p, seed, offset, 0,
        emb_w.data_ptr() if E else None, emb_b.data_ptr() if E else None, E, B, I, xin.data_ptr(), ldxin, xt.data_ptr(),
        xt.stride(0), temb.data_ptr() if E else None, None, st()))
    xt = xt.cpu().numpy()
    assert (xt[:, I:] == -3.0).all()
    return xin.cpu().numpy(), xt[:, :I]


def _check_builder(x, ts, p, E, offset):
    B, I = x.shape
    xin, xt = _builder(x, ts, p, E, offset)
    ref = CA[ts][:, None].astype(np.float64) * x + CB[ts][:, None].astype(np.float64) * R.normals(B, I, 0, SEED, offset)
    err = np.abs(xt - ref)
    assert (err <= NORMAL_TOL * CB[ts][:, None]).all(), (I, p, E, float((err / CB[ts][:, None]).max()))
    assert (xt != 0).all()  # (so that a zero of xin is a dropped element)
    keep = R.keep_mask(B, I, p, SEED, offset)
    np.testing.assert_array_equal(xin[:, :I] != 0, keep)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    np.testing.assert_array_equal(xin[:, :I][keep], (xt * scale)[keep])  # float32 product, bit for bit
    assert (xin[:, I + E] == 1.0).all() and (xin[:, I + E + 1:] == 0.0).all()


@pytest.mark.parametrize("I", [1, 3, 1023, 1025, 2049, 3075, 4097, 5125])
def test_dense_builder_noise_and_keep_mask(I):
    """x_t = ca x + cb normals within NORMAL_TOL |cb| (x small, cb a power of two: the float32 roundings of the sum stay far
    below that), the zero pattern of xin equals the model's keep-mask, kept entries are x_t / (1 - p) bit for bit."""
    B = 3
    rng = np.random.default_rng(I)
    x = rng.uniform(2.0 ** -7, 2.0 ** -6, size=(B, I)).astype(np.float32)
    ts = np.array([0, 1, 2], dtype=np.int64)
    for p in (0.5, 0.3, 0.0):
        for E in (0, 10):
            _check_builder(x, ts, p, E, offset=3 + E)


def _binary_rows(B, I, rng, density=0.1):
    x = (rng.random((B, I)) < density).astype(np.float32)
    x[:, 0], x[:, -1] = 1.0, 0.0
    if I > 1:
        x[:, 1] = 0.0
    return x


def _csr(x):
    indptr = np.concatenate([[0], np.cumsum((x != 0).sum(1))]).astype(np.int64)
    indices = np.nonzero(x)[1].astype(np.int32)
    return dev(indptr), dev(indices), dev(np.arange(x.shape[0], dtype=np.int64))


def test_csr_builder_keep_mask():
    """gdmcf_dnn_prep_input_csr_f32 at I = 5125: the same mask and x_t as the model.  ca = 1, cb = 2^-6 on {0,1} rows: x_t = 0
    would need a normal of exactly 0 or -64."""
    B, I, E, p, offset = 3, 5125, 10, 0.5, 11
    x = _binary_rows(B, I, np.random.default_rng(1))
    ip, ix, rows = _csr(x)
    ldxin = (I + E + 3) // 4 * 4 + 4
    xin = torch.full((B, ldxin), -3.0, dtype=torch.float32, device=DEV)
    ca, cb = dev(np.ones(3, np.float32)), dev(np.full(3, 2.0 ** -6, np.float32))
    ts = dev(np.array([0, 1, 2], dtype=np.int64))
    emb_w, emb_b, temb = torch.randn(E, E, device=DEV), torch.randn(E, device=DEV), torch.zeros(B, E, device=DEV)
    bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gdmcf_dnn_prep_input_csr_f32(
        ip.data_ptr(), ix.data_ptr(), rows.data_ptr(), ts.data_ptr(), ca.data_ptr(), cb.data_ptr(), 2, None, 0, 2, None, 0, p,
        SEED, offset, emb_w.data_ptr(), emb_b.data_ptr(), E, B, I, xin.data_ptr(), ldxin, temb.data_ptr(), bits.data_ptr(),
        bits.stride(0), st()))
    xin = xin.cpu().numpy()
    nz = R.normals(B, I, 0, SEED, offset)
    assert (nz != 0).all()
    keep = R.keep_mask(B, I, p, SEED, offset)
    np.testing.assert_array_equal(xin[:, :I] != 0, keep)
    ref = 2.0 * (x + 2.0 ** -6 * nz)
    assert (np.abs(xin[:, :I] - ref)[keep] <= 2.0 * NORMAL_TOL * 2.0 ** -6 + 2.0 ** -23).all()  # (+ the sum's float32 rounding, |x_t| < 2)


def _cat_params():
    return dev(np.array([1.0, 0.5, 0.25], np.float32)), dev(np.array([3.0], np.float32))  # z = x_t + .5 a + .25 b + 3 > 0


def test_cat_builder_keep_mask():
    """gdmcf_cat_prep_input_f32 at I = 5125: the zero pattern of dropout(cat_layer(x_t, xU)) is the model's keep-mask."""
    B, I, E, p, offset = 3, 5125, 10, 0.3, 12
    rng = np.random.default_rng(2)
    x = _binary_rows(B, I, rng)
    xU = (rng.random((B, 2 * I)) < 0.5).astype(np.float32)
    ldxin = (I + E + 3) // 4 * 4 + 4
    ldxt = (I + 3) // 4 * 4
    xin = torch.full((B, ldxin), -3.0, dtype=torch.float32, device=DEV)
    xt = torch.zeros(B, ldxt, dtype=torch.float32, device=DEV)
    ca, cb = dev(np.ones(3, np.float32)), dev(np.full(3, 2.0 ** -6, np.float32))
    ts = dev(np.array([0, 1, 2], dtype=np.int64))
    cw, cbias = _cat_params()
    emb_w, emb_b, temb = torch.randn(E, E, device=DEV), torch.randn(E, device=DEV), torch.zeros(B, E, device=DEV)
    xd, xUd = dev(x), dev(xU)
    _lib.check(_lib.load().gdmcf_cat_prep_input_f32(
        xd.data_ptr(), xd.stride(0), xUd.data_ptr(), xUd.stride(0), ts.data_ptr(), ca.data_ptr(), cb.data_ptr(), 2, None, 0, 2,
        None, 0, p, SEED, offset, cw.data_ptr(), cbias.data_ptr(), emb_w.data_ptr(), emb_b.data_ptr(), E, B, I, xin.data_ptr(),
        ldxin, xt.data_ptr(), ldxt, temb.data_ptr(), st()))
    xin, xt = xin.cpu().numpy(), xt.cpu().numpy()[:, :I]
    assert (np.abs(xt - (x + 2.0 ** -6 * R.normals(B, I, 0, SEED, offset))) <= NORMAL_TOL * 2.0 ** -6 + 2.0 ** -24).all()
    np.testing.assert_array_equal(xin[:, :I] != 0, R.keep_mask(B, I, p, SEED, offset))


# ---- class draws ----------------------------------------------------------------------------------------------------------------
def _onehot_noise(x, ts, discrete, seed, offset):
    B, I = x.shape
    xd, tsd = dev(x), dev(ts)
    xU = torch.full((B, 2 * I + 2), -3.0, dtype=torch.float32, device=DEV)
    so = torch.full((B, I + 1), 9, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().gdmcf_onehot_noise_f32(xd.data_ptr(), xd.stride(0), tsd.data_ptr(), B, I, discrete, None, 0, seed,
                                                  offset, xU.data_ptr(), xU.stride(0), so.data_ptr(), so.stride(0), st()))
    xU, so = xU.cpu().numpy(), so.cpu().numpy()
    assert (xU[:, 2 * I:] == -3.0).all() and (so[:, I:] == 9).all()
    return xU[:, :2 * I], so[:, :I]


@pytest.mark.parametrize("I", [1, 5, 1027, 4099])
def test_onehot_noise_classes(I):
    B = 4
    ts = np.array([0, B, 1, 3], dtype=np.int64)  # a = 0 and a = 1 among them
    x = _binary_rows(B, I, np.random.default_rng(I), density=0.4)
    c = (x != 0).astype(np.uint8)
    for discrete in (0.0, 0.3, 1.0):
        xU, s = _onehot_noise(x, ts, discrete, SEED, 21)
        ref = R.class_draws(c, ts, B, discrete, R.STREAM_ONEHOT_CLASS, SEED, 21)
        np.testing.assert_array_equal(s, ref)
        img = np.zeros((B, I, 2), dtype=np.float32)
        img[..., 0] = (c == 0) & (ref == 0)
        img[..., 1] = (c == 1) & (ref == 1)
        np.testing.assert_array_equal(xU, img.reshape(B, 2 * I))


def _unpack_bits(bits, I):
    w = bits.cpu().numpy().view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1)[:, :I].astype(np.uint8)


def test_csr_builders_draw_the_models_classes():
    """gdmcf_onehot_prep_input_csr_f32 (sampled_out) and gdmcf_cat_prep_input_csr_f32 (the class bitmap) at I = 1027: the
    classes of the model at offset_noise; the dropout of each at offset_prep (2I resp. I columns)."""
    B, I, E, p, discrete, off_noise, off_prep = 4, 1027, 10, 0.5, 0.3, 31, 32
    lib = _lib.load()
    x = _binary_rows(B, I, np.random.default_rng(3), density=0.4)
    ip, ix, rows = _csr(x)
    ts_U, ts = dev(np.array([0, B, 1, 3], dtype=np.int64)), dev(np.array([0, 1, 2, 0], dtype=np.int64))
    ref = R.class_draws(x != 0, np.array([0, B, 1, 3]), B, discrete, R.STREAM_ONEHOT_CLASS, SEED, off_noise)
    emb_w, emb_b, temb = torch.randn(E, E, device=DEV), torch.randn(E, device=DEV), torch.zeros(B, E, device=DEV)
    # one-hot builder
    ldxin = (2 * I + E + 3) // 4 * 4 + 4
    xin = torch.full((B, ldxin), -3.0, dtype=torch.float32, device=DEV)
    so = torch.full((B, I + 1), 9, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gdmcf_onehot_prep_input_csr_f32(
        ip.data_ptr(), ix.data_ptr(), rows.data_ptr(), ts_U.data_ptr(), discrete, None, 0, SEED, off_noise, so.data_ptr(),
        so.stride(0), ts.data_ptr(), 2, None, 0, p, off_prep, emb_w.data_ptr(), emb_b.data_ptr(), E, B, I, xin.data_ptr(), ldxin,
        temb.data_ptr(), None, 0, st()))
    so = so.cpu().numpy()
    np.testing.assert_array_equal(so[:, :I], ref)
    assert (so[:, I:] == 9).all()
    c = (x != 0)
    img = np.zeros((B, I, 2), dtype=bool)
    img[..., 0], img[..., 1] = ~c & (ref == 0), c & (ref == 1)
    keep = R.keep_mask(B, 2 * I, p, SEED, off_prep)
    want = np.where(img.reshape(B, 2 * I) & keep, np.float32(2.0), np.float32(0.0))  # kept bits of the image times 1 / (1 - p)
    np.testing.assert_array_equal(xin.cpu().numpy()[:, :2 * I], want)
    # cat builder
    ldxin, ldxt = (I + E + 3) // 4 * 4 + 4, (I + 3) // 4 * 4
    xin = torch.full((B, ldxin), -3.0, dtype=torch.float32, device=DEV)
    xt = torch.zeros(B, ldxt, dtype=torch.float32, device=DEV)
    ca, cb = dev(np.ones(3, np.float32)), dev(np.full(3, 2.0 ** -6, np.float32))
    cw, cbias = _cat_params()
    x0bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=DEV)
    clsbits = torch.zeros_like(x0bits)
    _lib.check(lib.gdmcf_cat_prep_input_csr_f32(
        ip.data_ptr(), ix.data_ptr(), rows.data_ptr(), ts_U.data_ptr(), discrete, None, 0, off_noise, ts.data_ptr(), ca.data_ptr(),
        cb.data_ptr(), 2, None, 0, 2, None, 0, p, SEED, off_prep, cw.data_ptr(), cbias.data_ptr(), emb_w.data_ptr(),
        emb_b.data_ptr(), E, B, I, xin.data_ptr(), ldxin, xt.data_ptr(), ldxt, temb.data_ptr(), x0bits.data_ptr(),
        x0bits.stride(0), clsbits.data_ptr(), clsbits.stride(0), st()))
    np.testing.assert_array_equal(_unpack_bits(clsbits, I), ref)
    np.testing.assert_array_equal(_unpack_bits(x0bits, I), c.astype(np.uint8))
    np.testing.assert_array_equal(xin.cpu().numpy()[:, :I] != 0, R.keep_mask(B, I, p, SEED, off_prep))


@pytest.mark.parametrize("user_guided", [0, 1])
@pytest.mark.parametrize("I", [5, 1027])
def test_graph_guided_step_draws(I, user_guided):
    B, discrete, offset = 4, 0.3, 41
    lib = _lib.load()
    rng = np.random.default_rng(I)
    g0 = (rng.random((B, I)) < 0.3).astype(np.uint8)
    g0[:, 0], g0[:, -1] = 1, 0
    ts = np.array([0, B, 1, 3], dtype=np.int64)
    degp = np.array([0.0, 1.0, 0.5, 0.25], dtype=np.float32)
    graph = torch.full((B, I + 3), 7, dtype=torch.uint8, device=DEV)
    graph[:, :I] = dev(g0)
    so = torch.full((B, I + 1), 9, dtype=torch.uint8, device=DEV)
    po = torch.full((B + 1,), 9, dtype=torch.uint8, device=DEV)
    tsd, dp = dev(ts), dev(degp)
    _lib.check(lib.gdmcf_graph_guided_step_u8(graph.data_ptr(), graph.stride(0), tsd.data_ptr(), B, I, discrete, None, 0, None,
                                              dp.data_ptr(), user_guided, SEED, offset, so.data_ptr(), so.stride(0), po.data_ptr(),
                                              st()))
    s = R.class_draws(g0, ts, B, discrete, R.STREAM_GRAPH_CLASS, SEED, offset)
    pick = R.graph_pick(degp, SEED, offset)
    assert pick[0] == 0 and pick[1] == 1  # degree_prob 0 and 1
    so, po, graph = so.cpu().numpy(), po.cpu().numpy(), graph.cpu().numpy()
    np.testing.assert_array_equal(so[:, :I], s)
    np.testing.assert_array_equal(po[:B], pick)
    gate = pick[:, None] if user_guided else np.ones((B, 1), dtype=np.uint8)
    np.testing.assert_array_equal(graph[:, :I], g0 | (s & gate))
    assert (so[:, I:] == 9).all() and po[B] == 9 and (graph[:, I:] == 7).all()


# ---- timesteps ------------------------------------------------------------------------------------------------------------------
def _sample_ts(hist, cnt, T, H, B, seed, offset, uniform_prob=0.001):
    ts = torch.full((B + 1,), -5, dtype=torch.int64, device=DEV)
    pt = torch.full((B + 1,), -5.0, dtype=torch.float64, device=DEV)
    p_out = torch.full((T,), -5.0, dtype=torch.float64, device=DEV)
    _lib.check(_lib.load().gdmcf_sample_timesteps(hist.data_ptr(), cnt.data_ptr(), T, H, B, uniform_prob, seed, offset,
                                                  ts.data_ptr(), pt.data_ptr(), p_out.data_ptr(), st()))
    ts, pt = ts.cpu().numpy(), pt.cpu().numpy()
    assert ts[B] == -5 and pt[B] == -5.0
    return ts[:B], pt[:B], p_out.cpu().numpy()


@pytest.mark.parametrize("T,B", [(1, 5), (2, 257), (40, 4096), (1000, 300)])
def test_sample_timesteps_draws(T, B):
    H, offset = 10, 51
    hist = torch.zeros(T, H, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(T, dtype=torch.int64, device=DEV)
    cnt[: T // 2] = H  # not every term full: the uniform branch
    ts, pt, p_out = _sample_ts(hist, cnt, T, H, B, SEED, offset)
    np.testing.assert_array_equal(ts, R.timesteps(B, T, SEED, offset))
    assert (pt == 1.0).all() and (p_out == -5.0).all()
    # importance branch: ts through the model from the kernel's own probabilities
    h = np.random.default_rng(T).uniform(0.01, 1.0, size=(T, H)) * np.linspace(0.2, 3.0, T)[:, None]
    hist.copy_(dev(h))
    cnt[:] = H
    ts, pt, p_out = _sample_ts(hist, cnt, T, H, B, SEED, offset + 1)
    w = np.sqrt((h ** 2).mean(axis=1))
    np.testing.assert_allclose(p_out, w / w.sum() * (1 - 0.001) + 0.001 / T, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(ts, R.timesteps(B, T, SEED, offset + 1, p=p_out))
    np.testing.assert_array_equal(pt, p_out[ts] * float(T))


# ---- BPR triples ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 257])
def test_bpr_sample_draws(B):
    n_items, offset = 50, 61
    rng = np.random.default_rng(B)
    degs = [0, 1, 49, 50, 7, 20]
    rows = [np.sort(rng.choice(n_items, size=d, replace=False)).astype(np.int32) for d in degs]
    indptr = np.concatenate([[0], np.cumsum(degs)]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    n_users = len(degs)
    if B == 1:
        users = np.array([4], dtype=np.int64)
    else:
        users = (np.arange(B) % n_users).astype(np.int64)
        users[100] = n_users  # out of range
        users[101] = -1
    ip, ix, ud = dev(indptr), dev(indices), dev(users)
    pos = torch.full((B + 1,), -9, dtype=torch.int64, device=DEV)
    neg = torch.full((B + 1,), -9, dtype=torch.int64, device=DEV)
    flag = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gdmcf_bpr_sample_f32(ip.data_ptr(), ix.data_ptr(), ud.data_ptr(), B, n_users, n_items, SEED, offset,
                                                pos.data_ptr(), neg.data_ptr(), flag.data_ptr(), st()))
    rp, rn, rf = R.bpr_triples(indptr, indices, users, n_users, n_items, SEED, offset)
    assert rf == (0 if B == 1 else 1)
    np.testing.assert_array_equal(pos.cpu().numpy(), np.append(rp, -9))
    np.testing.assert_array_equal(neg.cpu().numpy(), np.append(rn, -9))
    assert flag.cpu().tolist() == [rf, 0]


# ---- the offset's high bits -------------------------------------------------------------------------------------------------------
def test_offsets_that_differ_above_bit_31_draw_differently():
    """Offsets 5 and 2^40 + 5: different normals, keep-masks and classes, each equal to the model's at its own offset."""
    lo, hi = 5, (1 << 40) + 5
    rows, cols = 3, 1027
    a, b = randn(rows, cols, cols, 0, SEED, lo), randn(rows, cols, cols, 0, SEED, hi)
    assert not np.array_equal(a, b)
    for got, off in ((a, lo), (b, hi)):
        assert np.abs(got - R.normals(rows, cols, 0, SEED, off)).max() <= NORMAL_TOL
    x = np.random.default_rng(0).uniform(2.0 ** -7, 2.0 ** -6, size=(3, 2049)).astype(np.float32)
    ts = np.array([0, 1, 2], dtype=np.int64)
    ka, kb = (_builder(x, ts, 0.5, 0, off)[0][:, :2049] != 0 for off in (lo, hi))
    assert not np.array_equal(ka, kb)
    np.testing.assert_array_equal(ka, R.keep_mask(3, 2049, 0.5, SEED, lo))
    np.testing.assert_array_equal(kb, R.keep_mask(3, 2049, 0.5, SEED, hi))
    B, I = 4, 1027
    xb = _binary_rows(B, I, np.random.default_rng(1), density=0.4)
    tsU = np.array([0, B, 1, 3], dtype=np.int64)
    sa, sb = (_onehot_noise(xb, tsU, 0.3, SEED, off)[1] for off in (lo, hi))
    assert not np.array_equal(sa, sb)
    np.testing.assert_array_equal(sa, R.class_draws(xb != 0, tsU, B, 0.3, 3, SEED, lo))
    np.testing.assert_array_equal(sb, R.class_draws(xb != 0, tsU, B, 0.3, 3, SEED, hi))
    # the largest offset the counter carries
    top = (1 << 56) - 1
    assert np.abs(randn(2, 5, 8, 4, SEED, top)[:, :5] - R.normals(2, 5, 4, SEED, top)).max() <= NORMAL_TOL


def test_q_sample_and_the_engine_builder_do_not_share_noise():
    """q_sample call n draws at offset 2^40 + n, the engine's builder of step n at offset n, both keyed by the same seed: their
    stream-0 normals differ."""
    torch.manual_seed(1234)
    B, I = 4, 1027
    m = gdmcf_amd.DNN([I, 16], [16, I], 10).to(DEV)
    d = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear", 1.0, 0.5, 0.5, 4, DEV)
    eng = m.engine
    assert eng.seed == int(torch.initial_seed())
    bufs = eng.buffers(B, torch.device(DEV))
    x0 = torch.zeros(B, I, device=DEV)
    ts = torch.arange(B, device=DEV) % 4
    ca, cb = d._t32["sqrt_ab"], d._t32["sqrt_1mab"]
    xt = torch.zeros(B, I, device=DEV)
    for n in (1, 2):
        q = d.q_sample(x0, ts)
        assert d._q_calls == n
        eng._prep_input(bufs, x0, I, bufs.xin, ts, ca, cb, None, None, False, xt_out=xt)
        assert eng.offset == n
        assert not torch.equal(q, xt), f"q_sample call {n} repeats the noise of the builder at offset {n}"
        cbv = cb[ts].double().cpu().numpy()[:, None]
        seed = int(torch.initial_seed())
        assert (np.abs(q.cpu().numpy() - cbv * R.normals(B, I, 0, seed, (1 << 40) + n)) <= NORMAL_TOL * cbv + 2.0 ** -22).all()
        assert (np.abs(xt.cpu().numpy() - cbv * R.normals(B, I, 0, seed, n)) <= NORMAL_TOL * cbv + 2.0 ** -22).all()


# ---- production path against injected path -----------------------------------------------------------------------------------------
def _production_pair(kind):
    B, I, T, discrete = 5, 1100, 4, 0.3
    torch.manual_seed(4321)
    seed = int(torch.initial_seed())
    if kind == "dnn":
        m = gdmcf_amd.DNN([I, 16], [16, I], 10)
        d = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear", 1.0, 0.5, 0.5, T, DEV)
    else:
        m = (gdmcf_amd.DNNOneHot if kind == "onehot" else gdmcf_amd.DNNCat)([I, 16], [16, I], 10)
        d = gdmcf_amd.GaussianDiffusionDiscrete(ModelMeanType.START_X, "linear", 1.0, 0.5, 0.5, T, DEV, discrete=discrete,
                                                CatOneHot=True)
    m = m.to(DEV).train()
    assert m.drop.p == 0.5
    m.engine.manual_seed(seed)
    x = _binary_rows(B, I, np.random.default_rng(7), density=0.3)
    return m, d, x, seed, (B, I, T, discrete)


@pytest.mark.parametrize("kind", ["dnn", "onehot", "cat"])
def test_production_step_equals_the_step_with_the_models_draws_injected(kind):
    """One training_losses with every draw made in the kernels, then the same step with the draws handed in: timesteps, keep-masks
    and classes from the host model, the noise from gdmcf_randn_f32 at the builder's (seed, offset).  Equal losses, bit for bit,
    pin which offset and stream each draw of a step consumes (the injected path is pinned to the reference fixtures elsewhere)."""
    m, d, x, seed, (B, I, T, discrete) = _production_pair(kind)
    xd = dev(x)
    with torch.no_grad():
        l1 = d.training_losses(m, xd, True)["loss"].clone()
    eng = m.engine
    # timesteps: history empty -> the uniform branch, pt = 1; the one-hot variants draw ts_U first
    n_ts = 1 if kind == "dnn" else 2
    assert d._ts_calls == n_ts
    ts = R.timesteps(B, T, seed, n_ts)
    np.testing.assert_array_equal(d.last_ts.cpu().numpy(), ts)
    inj = dict(ts=dev(ts), pt=torch.ones(B, dtype=torch.float64, device=DEV))
    if kind == "dnn":  # one builder: noise (stream 0) and dropout (stream 1) at offset 1
        assert eng.offset == 1
        off_b = 1
    else:  # class draws (stream 3) at offset 1, the builder(s) behind them
        assert eng.offset == (3 if kind == "onehot" else 2)
        ts_U = R.timesteps(B, T, seed, 1)
        inj.update(ts_U=dev(ts_U), sampled=dev(R.class_draws(x != 0, ts_U, B, discrete, R.STREAM_ONEHOT_CLASS, seed, 1)))
        off_b = 2
        if kind == "onehot":  # the second branch's dropout over the [B, 2I] image at offset 3
            inj.update(drop_mask_U=dev(R.keep_mask(B, 2 * I, 0.5, seed, 3).astype(np.uint8)))
    inj.update(noise=_lib.philox_randn((B, I), DEV, seed, off_b, stream_id=0),
               drop_mask=dev(R.keep_mask(B, I, 0.5, seed, off_b).astype(np.uint8)))
    with torch.no_grad():
        l2 = d.training_losses(m, xd, True, **inj)["loss"]
    assert bool(torch.isfinite(l1).all()) and float(l1.abs().min()) > 0
    assert torch.equal(l1, l2), (l1.tolist(), l2.tolist())
