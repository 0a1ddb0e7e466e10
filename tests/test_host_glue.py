"""CPU (-m "not gpu"): the host side of the glue-kernel tests (tests/glue_ref.py and the GPU modules test_gpu_rows.py,
test_gpu_adamw.py, test_gpu_loss_tail.py, test_gpu_dp_pack.py).  The C entries of csrc/rows.hip, adamw.hip, loss_tail.hip,
dp_exchange.hip and gdmcf_rowscale_f32 must refuse bad sizes with GDMCF_E_SHAPE and bad values / missing pointers with
GDMCF_E_ARG -- every call here returns before a launch -- and the reference module must be right on cases worked out by hand."""
import ctypes
import math

import numpy as np
import pytest

from gdmcf_amd import _lib
from tests import glue_ref as R

P = 4096  # a non-NULL pointer that is never followed: every call below fails a check first
OK, E_SHAPE, E_ARG = _lib.GDMCF_OK, _lib.E_SHAPE, _lib.E_ARG


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, name, defaults, **change):
    args = dict(defaults, **change)
    assert set(change) <= set(defaults), (name, change)
    return getattr(lib, name)(*args.values())


def _sweep(lib, name, defaults, shape=(), arg=(), required=()):
    """Each change of `shape` must give E_SHAPE, each of `arg` E_ARG, and each pointer of `required` set to NULL E_ARG."""
    for change in shape:
        assert _call(lib, name, defaults, **change) == E_SHAPE, (name, change)
    for change in arg:
        assert _call(lib, name, defaults, **change) == E_ARG, (name, change)
    for ptr in required:
        assert defaults[ptr] == P, (name, ptr)
        assert _call(lib, name, defaults, **{ptr: None}) == E_ARG, (name, ptr)
        assert lib.gdmcf_last_error().decode(), (name, ptr)  # the refusal names its reason


# ---- csrc/rows.hip and rowscale --------------------------------------------------------------------------------------------------
def test_row_norms_and_normalize_rows_bwd_refuse(lib):
    d = dict(X=P, ld=8, rows=3, cols=8, norm=P, inv=P, stream=None)
    _sweep(lib, "gdmcf_row_norms_f32", d, shape=[dict(rows=0), dict(rows=-1), dict(cols=0), dict(ld=7)],
           arg=[dict(norm=None, inv=None)], required=["X"])
    d = dict(dY=P, lddy=8, Y=P, ldy=8, rn=P, rows=3, cols=8, dX=P, lddx=8, stream=None)
    _sweep(lib, "gdmcf_normalize_rows_bwd_f32", d,
           shape=[dict(rows=0), dict(cols=0), dict(cols=-4), dict(lddy=7), dict(ldy=7), dict(lddx=7)],
           required=["dY", "Y", "rn", "dX"])


def test_tanh_bwd_gather_and_scatter_refuse(lib):
    d = dict(dA=P, ldd=8, A=P, lda=8, extra=P, lde=8, scale=P, M=2, N=8, out=P, ldo=8, stream=None)
    _sweep(lib, "gdmcf_tanh_bwd_f32", d,
           shape=[dict(M=0), dict(N=0), dict(ldd=7), dict(lda=7), dict(ldo=7), dict(lde=7)],
           arg=[dict(scale=None)], required=["dA", "A", "out"])
    assert _call(lib, "gdmcf_tanh_bwd_f32", d, extra=None, lde=0, dA=None) == E_ARG  # lde is not read without `extra`
    for name in ("gdmcf_gather_rows_f32", "gdmcf_scatter_add_rows_f32"):
        d = dict(src=P, lds=8, index=P, n=3, cols=8, dst=P, ldd=8, stream=None)
        _sweep(lib, name, d, shape=[dict(n=0), dict(n=-2), dict(cols=0), dict(lds=7), dict(ldd=7)],
               required=["src", "index", "dst"])


def test_emb_bwd_densify_scale_and_rowscale_refuse(lib):
    d = dict(dZ1=P, lddz=8, W1=P, ldw=20, I=10, E=10, temb=P, M=4, N=8, ws=P, dWe=P, dbe=P, stream=None)
    _sweep(lib, "gdmcf_emb_bwd_f32", d,
           shape=[dict(M=0), dict(N=0), dict(E=0), dict(E=-1), dict(I=-1), dict(ldw=19), dict(lddz=7)],
           required=["dZ1", "W1", "temb", "ws", "dWe", "dbe"])
    d = dict(indptr=P, indices=P, values=P, row_ids=P, B=2, I=8, out=P, ldo=8, stream=None)
    _sweep(lib, "gdmcf_densify_rows_f32", d, shape=[dict(B=0), dict(I=0), dict(I=-3), dict(ldo=7)],
           required=["indptr", "indices", "out"])
    assert _call(lib, "gdmcf_densify_rows_f32", d, values=None, row_ids=None, out=None) == E_ARG  # both optional: `out` refused
    d = dict(acc=P, n=5, scale=2.0, out=P, stream=None)
    _sweep(lib, "gdmcf_scale_f32", d, shape=[dict(n=0), dict(n=-1)], required=["acc", "out"])
    d = dict(A=P, lda=8, rs=P, M=2, K=8, out=P, ldo=8, stream=None)
    _sweep(lib, "gdmcf_rowscale_f32", d, shape=[dict(M=0), dict(K=0), dict(lda=7), dict(ldo=7)])


# ---- csrc/loss_tail.hip ----------------------------------------------------------------------------------------------------------
_FINISH = dict(rowsum=P, rowdiv=P, alpha=P, ts=P, weight=P, pt=P, B=8, T=5, H=3, hist=P, cnt=P, update=1, lu=P, loss=P,
               gradcoef=P)


def test_row_loss_finish_refuses(lib):
    required = ["rowsum", "rowdiv", "ts", "weight", "pt", "lu", "loss"]
    for name, d in (("gdmcf_row_loss_finish_f64", dict(_FINISH, stream=None)),
                    ("gdmcf_row_loss_finish_mean_f64", dict(_FINISH, loss_mean=P, rowscale_mean=P, stream=None))):
        _sweep(lib, name, d, shape=[dict(B=0), dict(T=0), dict(H=0), dict(B=-1)],
               arg=[dict(T=2000, H=10)],  # 160 KB of history: above the 150 KiB the LDS-resident FIFO update may ask for
               required=required + ["hist", "cnt"])  # update_history = 1 needs the history
        for update in (0, 1):  # the other pointers are required either way, also with every optional one absent
            for ptr in required:
                assert _call(lib, name, d, update=update, alpha=None, **{ptr: None}) == E_ARG, (name, update, ptr)
    d = dict(_FINISH, loss_mean=P, rowscale_mean=P, stream=None)
    assert _call(lib, "gdmcf_row_loss_finish_mean_f64", d, gradcoef=None) == E_ARG  # rowscale_mean without gradcoef
    assert b"rowscale_mean" in lib.gdmcf_last_error()
    # update_history = 0 does not need the history: the refusal below is the LDS limit's, after the pointer checks have passed
    assert _call(lib, "gdmcf_row_loss_finish_mean_f64", d, update=0, hist=None, cnt=None, T=2000, H=10) == E_ARG
    assert b"LDS" in lib.gdmcf_last_error()


def test_lt_history_update_refuses(lib):
    d = dict(ts=P, lu=P, B=8, T=5, H=3, hist=P, cnt=P, stream=None)
    _sweep(lib, "gdmcf_lt_history_update", d, shape=[dict(B=0), dict(T=0), dict(H=0)], arg=[dict(T=2000, H=10)],
           required=["ts", "lu", "hist", "cnt"])


# ---- csrc/dp_exchange.hip --------------------------------------------------------------------------------------------------------
def test_dp_pack_and_unpack_refuse(lib):
    grads = (ctypes.c_void_p * 17)(*([P] * 17))
    counts = (ctypes.c_int64 * 17)(*([3] * 17))
    g, c = ctypes.addressof(grads), ctypes.addressof(counts)
    d = dict(grads=g, counts=c, n=2, ts=P, lu=P, B=4, rank=0, world=2, flat=P, stream=None)
    _sweep(lib, "gdmcf_dp_pack_f64", d,
           shape=[dict(n=17), dict(n=-1), dict(B=0), dict(world=0), dict(rank=2), dict(rank=5), dict(rank=-1)],
           arg=[dict(grads=None), dict(counts=None)], required=["ts", "lu", "flat"])
    d = dict(flat=P, grads=g, counts=c, n=2, B=4, world=2, ts_all=P, lu_all=P, stream=None)
    _sweep(lib, "gdmcf_dp_unpack_f64", d, shape=[dict(n=17), dict(n=-1), dict(B=0), dict(world=0)],
           arg=[dict(grads=None), dict(counts=None)], required=["flat", "ts_all", "lu_all"])
    # the table itself: a negative count, and a NULL gradient with a count above zero (a NULL with count 0 is allowed)
    for bad_grads, bad_counts in (([P, P], [3, -1]), ([P, None], [3, 2])):
        gg, cc = (ctypes.c_void_p * 2)(*bad_grads), (ctypes.c_int64 * 2)(*bad_counts)
        assert lib.gdmcf_dp_pack_f64(ctypes.addressof(gg), ctypes.addressof(cc), 2, P, P, 4, 0, 2, P, None) == E_ARG
        assert lib.gdmcf_dp_unpack_f64(P, ctypes.addressof(gg), ctypes.addressof(cc), 2, 4, 2, P, P, None) == E_ARG


# ---- csrc/adamw.hip --------------------------------------------------------------------------------------------------------------
def test_adamw_refuses(lib):
    d = dict(table=P, n=1, blocks=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=1, gs=1.0, stream=None)
    _sweep(lib, "gdmcf_adamw_f32", d, arg=[dict(step=0), dict(step=-1), dict(n=0), dict(blocks=0)])
    d = dict(table=P, shadow=P, n=1, blocks=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=1, gs=1.0, stream=None)
    _sweep(lib, "gdmcf_adamw_bf16s_f32", d, arg=[dict(shadow=None), dict(step=0)])


# ---- tests/glue_ref.py on cases worked out by hand --------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.LOSS_B)
def test_kernel_mean_emulation_against_fsum(B):
    """The butterfly order within B * 2^-53 * sum |loss| of the exactly rounded mean, at every batch size of the GPU cases."""
    for T, _ in R.LOSS_TH:
        loss = R.row_loss(*R.loss_case(B, T, seed=B))[1]
        exact = math.fsum(loss.tolist()) / B
        assert abs(R.kernel_mean(loss) - exact) * B <= R.kernel_mean_bound(loss)
        assert abs(R.kernel_mean(loss, "pairs") - exact) * B <= R.kernel_mean_bound(loss)


def test_kernel_mean_order_by_hand_and_told_apart_by_the_test_data():
    """Thread t owns rows t, t + 256, ...: with 2^60 in row 0, 1.0 in rows 256 and 512 and -2^60 in row 64 the ones are absorbed
    (2^60 + 1 == 2^60), whereas any order that adds the ones first keeps them.  And the data of the GPU cases distinguish the
    kernel's ((s0 + s1) + s2) + s3 from (s0 + s2) + (s1 + s3) at several batch sizes."""
    x = np.zeros(513)
    x[0], x[256], x[512], x[64] = 2.0 ** 60, 1.0, 1.0, -2.0 ** 60
    assert R.kernel_mean(x) == 0.0 and math.fsum(x.tolist()) == 2.0
    y = np.zeros(256)
    y[0], y[64], y[128], y[192] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -52  # waves 0 .. 3
    assert R.kernel_mean(y) * 256 == 1.0 + 2.0 ** -52  # ((1 + 2^-53) + 2^-53) + 2^-52: both halves lost to ties-to-even
    assert R.kernel_mean(y, "pairs") * 256 == 1.0 + 2.0 ** -51  # (1 + 2^-53) + (2^-53 + 2^-52) rounds up
    differ = [B for B in R.LOSS_B for T, _ in R.LOSS_TH
              if R.kernel_mean(R.row_loss(*R.loss_case(B, T, seed=B))[1]) !=
              R.kernel_mean(R.row_loss(*R.loss_case(B, T, seed=B))[1], "pairs")]
    assert len(set(differ)) >= 2 and min(differ) > 128, differ  # (up to 128 rows only waves 0 and 1 hold anything)


def test_row_loss_by_hand():
    lu, loss, gc, rsm = R.row_loss([6.0, 1.0], [4.0, 3.0], [0.5, 2.0], [1, 0], [10.0, 0.25], [2.0, 0.5])
    third = np.float64(np.float32(1.0) / np.float32(3.0))
    assert lu.tolist() == [0.25 * 1.5, 10.0 * third] and loss.tolist() == [0.25 * 1.5 / 2.0, 10.0 * third / 0.5]
    assert gc.dtype == rsm.dtype == np.float32
    assert gc.tolist() == [np.float32(2.0 * 0.5 * 0.25 / (2.0 * 4.0)), np.float32(2.0 * 2.0 * 10.0 / (0.5 * 3.0))]
    assert rsm.tolist() == [g * np.float32(0.5) for g in gc]
    assert R.row_loss([6.0], [4.0], None, [0], [3.0], [1.0])[2].tolist() == [1.5]  # alpha absent: 2 * 1 * 3 / (1 * 4)


def test_densify_and_the_csr_case_by_hand():
    indptr, indices = np.array([0, 3, 3, 5]), np.array([2, -1, 4, 0, 3], dtype=np.int32)
    vals = np.array([5.0, 6.0, 7.0, 8.0, 9.0], dtype=np.float32)
    assert R.densify(indptr, indices, None, None, 3, 4).tolist() == [[0, 0, 1, 0], [0, 0, 0, 0], [1, 0, 0, 1]]
    assert R.densify(indptr, indices, vals, [2, 0], 2, 4).tolist() == [[8, 0, 0, 9], [0, 0, 5, 0]]
    for I in (1, 3, 1030):
        ip, ix = R.csr_case(I, seed=0)
        deg = np.diff(ip)
        assert len(deg) == 9 and deg[1] == 0 and deg[2] == I and deg[4] == 3 and deg[6] == I + 3
        for r in range(9):
            row = ix[ip[r]:ip[r + 1]]
            ok = row[(row >= 0) & (row < I)]
            assert len(np.unique(ok)) == len(ok)  # each valid column at most once
        assert {-1, I, I + 5} <= set(ix.tolist())
        dense = R.densify(ip, ix, None, R.ROW_IDS, len(R.ROW_IDS), I)
        assert dense[5].all() and not dense[6].any()  # row 2 full, row 1 empty
    assert sorted(R.ROW_IDS, reverse=True) == list(R.ROW_IDS) and len(set(R.ROW_IDS)) < len(R.ROW_IDS)


def test_bounds_by_hand():
    u = R.U
    assert u == 2.0 ** -24
    # tanh_bwd: 4u (|dA| + |scale extra|)
    assert R.tanh_bwd_bound([[2.0, -3.0]]).tolist() == [[8 * u, 12 * u]]
    assert R.tanh_bwd_bound([[2.0]], [[-4.0]], 0.5).tolist() == [[16 * u]]
    assert R.tanh_bwd_ref([[2.0]], [[0.5]], [[-4.0]], 0.5).tolist() == [[0.0]] and R.tanh_bwd_ref([[2.0]], [[0.5]]).tolist() == [[1.5]]
    # row_norms: d = 4 ceil(cols / 1024) + 9; norm (d / 2 + 2) u, inverse one more
    assert [R.row_norms_depth(c) for c in (1, 1024, 1025, 4099)] == [13, 13, 17, 29]
    assert R.row_norms_rel_bound(1024) == 8.5 * u and R.row_norms_rel_bound(4099, inverse=True) == 17.5 * u
    # normalize_rows_bwd: d = 13 on the register branch, ceil(cols / 256) + 9 on the two-pass branch
    assert [R.normalize_bwd_depth(c) for c in (4, 4096, 1, 97, 4097, 4100, 5000)] == [13, 13, 10, 10, 26, 26, 29]
    dY, Y, rn = np.array([[1.0, 2.0, 0.0, 0.0]]), np.array([[0.5, 0.25, 0.0, 1.0]]), np.array([2.0])
    # dot = 1, sum |dy y| = 1: dX = (dY - Y) * 2; bound = 2 (|Y| 15u + 3u (|dY| + |Y|))
    assert R.normalize_bwd_ref(dY, Y, rn).tolist() == [[1.0, 3.5, 0.0, -2.0]]
    assert np.allclose(R.normalize_bwd_bound(dY, Y, rn), 2 * u * np.array([[7.5 + 4.5, 3.75 + 6.75, 0.0, 15.0 + 3.0]]), rtol=1e-15)
    # emb_bwd: (ceil(N / 64) + ceil(M / 64) + 16) u = 18u at M = N = 2
    dZ, W1, temb = np.array([[1.0, -2.0], [3.0, 4.0]]), np.array([[9.0, 1.0], [9.0, -1.0]]), np.array([[2.0], [-1.0]])
    demb, dWe, dbe = R.emb_bwd_ref(dZ, W1, 1, 1, temb, 2)
    assert demb.tolist() == [[3.0], [-1.0]] and dWe.tolist() == [[7.0]] and dbe.tolist() == [2.0]
    bd, bw, bb = R.emb_bwd_bounds(dZ, W1, 1, 1, temb, 2)
    assert bd.tolist() == [[54 * u], [126 * u]] and bw.tolist() == [[18 * u * 13]] and bb.tolist() == [18 * u * 10]
    assert R.emb_bwd_bounds(np.ones((130, 200)), np.ones((200, 47)), 37, 10, np.ones((130, 10)), 200)[0][0, 0] == (4 + 3 + 16) * u * 200
    # AdamW: m 2u (|m0| + |g|), v 3u (|v0| + g^2) with the scaled gradient; p without decay and with m0 = g (no propagated term
    # beyond 2u |g| lr / bc1 / denom)
    h = dict(lr=0.5, beta1=0.5, beta2=0.75, eps=0.0, weight_decay=0.0, step=1, grad_scale=0.5)
    p64, m64, v64, term, gs = R.adam64([1.0], [4.0], [2.0], [4.0], **h)
    assert (gs.tolist(), m64.tolist(), v64.tolist()) == ([2.0], [2.0], [4.0])  # denom = 2 / sqrt(0.25) = 4, term = 0.5 / 0.5 * 2 / 4
    assert term.tolist() == [0.5] and p64.tolist() == [0.5]
    bp, bm, bv = R.adam_bounds([1.0], [4.0], [2.0], [4.0], **h)
    assert bm.tolist() == [8 * u] and bv.tolist() == [24 * u]
    assert np.allclose(bp, 2 * u * 0.5 + R.ADAM_C * 0.5 + 8 * u * (0.5 / 0.5 / 4.0), rtol=1e-15)
    assert R.adam_bound_p_as_first_stated([1.0], [4.0], [2.0], [4.0], **h).tolist() == [2 * u * 0.5 + R.ADAM_C * 0.5]
    assert R.adam_table([0, 1, 4096, 0, 4097, 0]) == ([0, 0, 1, 2, 2, 4], 4)


@pytest.mark.parametrize("hyper", R.ADAM_HYPERS, ids=lambda h: f"step{h['step']}-lr{h['lr']}")
def test_adam_bounds_hold_for_a_correctly_rounded_float32_evaluation(hyper):
    """gd_adam_elem's operations in numpy float32 (reciprocal and square root correctly rounded) stay inside the three bounds on a
    million elements of the GPU cases' distribution, using less than half of ADAM_C."""
    p, g, m, v = R.adam_state(1 << 20, seed=1)
    p64, m64, v64, term, _ = R.adam64(p, g, m, v, **hyper)
    bp, bm, bv = R.adam_bounds(p, g, m, v, **hyper)
    pf, mf, vf = R.adam_f32(p, g, m, v, **hyper)
    assert (np.abs(pf - p64) <= bp).all() and (np.abs(mf - m64) <= bm).all() and (np.abs(vf - v64) <= bv).all()
    half = bp - 0.5 * R.ADAM_C * np.abs(term)
    assert (np.abs(pf - p64) <= half).all()


def test_parameter_bound_needs_the_two_added_terms():
    """Without d_decay and m's propagated error the parameter bound is too small for float32 arithmetic itself: the correctly
    rounded evaluation leaves it at the sizes of the GPU cases (glue_ref.adam_bounds says why)."""
    over = 0
    for hyper in R.ADAM_HYPERS:
        for n in R.ADAM_NUMELS:
            p, g, m, v = R.adam_state(n, seed=1)
            p64 = R.adam64(p, g, m, v, **hyper)[0]
            over += int((np.abs(R.adam_f32(p, g, m, v, **hyper)[0] - p64) > R.adam_bound_p_as_first_stated(p, g, m, v, **hyper)).sum())
    assert over > 0
