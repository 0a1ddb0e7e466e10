"""GPU (-m gpu): gdmcf_bpr_loss_f32 and gdmcf_bpr_grad_f32 (csrc/bpr.hip) on their own, through the C ABI with raw pointers and
leading dimensions, against the float64 reference of tests/bpr_ref.py -- no model, no graph, no propagation (the step as a whole
is tests/test_gpu_bpr.py's).  Every lane-group size 1 .. 64 and one to three column passes; runs of exactly LG and 2 LG entries,
a run that ends at entry 3 B - 1, one that crosses a workgroup's last lane group, adjacent nodes, out-of-range ids whose sort keys
touch a valid run; mode 1 with and without zero_rows; strides, alignments and the flag pointer.

Operands are windows [:, :d] of wider buffers with guard rows around them: NaN outside the window for inputs, a NaN with a payload
for outputs, and after every call each buffer is compared whole -- what the contract does not name keeps its bits.  On dyadic
tables (tests/bpr_ref.py) x, rg, reg and every scatter row are exact, so they are held bit for bit; real tables are held to the
bounds derived there.

The one measured tolerance: with x exact, coef = sigmoid(x) / B and soft = softplus(x) carry only the device's expf, log1pf and
divisions.  Over all cases of test_loss (18 widths, 9 batches, 2 tables, x from -80 to beyond 20 on both sides) an MI355X with
ROCm 7 gave max |coef / ref - 1| = 2.156 * 2^-24 and max |soft / ref - 1| = 1.234 * 2^-24 against float64 (test_loss prints the
figures of every width).  COEF_TOL and SOFT_TOL are four times those, room for another libm; tests/bpr_ref.py refuses anything
above 16 * 2^-24."""
import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from tests import bpr_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
COEF_SEEN, SOFT_SEEN = 2.156 * R.U, 1.234 * R.U  # measured, see above
TRANS_TOL = (4 * COEF_SEEN, 4 * SOFT_SEEN)  # (COEF_TOL, SOFT_TOL)
NAN_BITS, SENTINEL = 0x7FC00000, 0x7FC5BEE5  # a quiet NaN; one with a payload no arithmetic produces
GUARD = 2  # rows of the buffer's fill before and after the window
SCALE = 2.0 ** -7


class Seat:
    """A [rows, d] window of row stride ld, `off` floats behind an aligned address plus GUARD rows, in a buffer of `fill` bits"""

    def __init__(self, rows, d, ld=None, off=0, data=None, fill=NAN_BITS):
        self.rows, self.d, self.ld = rows, d, d + 4 if ld is None else ld
        assert self.ld >= d
        self.start = off + GUARD * self.ld
        host = np.full(self.start + (rows + GUARD) * self.ld + 4, fill, np.int32)
        if data is not None:
            self.window(host)[:] = np.ascontiguousarray(data, F32).reshape(rows, d).view(np.int32)
        self.host0 = host
        self.dev = torch.from_numpy(host.copy()).to(DEV)
        self.ptr = self.dev.data_ptr() + 4 * self.start
        assert self.dev.data_ptr() % 16 == 0

    def window(self, host):
        return np.lib.stride_tricks.as_strided(host[self.start:], (self.rows, self.d), (4 * self.ld, 4))

    def initial(self):
        return self.window(self.host0).copy().view(F32)

    def values(self):
        """the window now; everything outside it must be as it was"""
        now = self.dev.cpu().numpy()
        got = self.window(now).copy()
        self.window(now)[:] = self.window(self.host0)
        assert np.array_equal(now, self.host0), "written outside the window"
        return got.view(F32)

    def untouched(self):
        return np.array_equal(self.dev.cpu().numpy(), self.host0)


def ids_of(b):
    return [torch.from_numpy(a).to(DEV) for a in (b.users, b.pos, b.neg)]


def vec(n, data=None, fill=SENTINEL):
    return Seat(1, n, n + 3, data=data, fill=fill)


def run_loss(Ms, Es, b, with_flag=True):
    """(coef [B], ws [2B], mf, reg, flag) of one call; every buffer checked around its window, the inputs whole"""
    lib, B = _lib.load(), b.B
    ids = ids_of(b)
    coef, ws, mf, reg = vec(B), vec(2 * B), vec(1), vec(1)
    flag = torch.tensor([SENTINEL, 0, SENTINEL], dtype=torch.int32, device=DEV)
    rc = lib.gdmcf_bpr_loss_f32(Ms.ptr, Ms.ld, Es.ptr, Es.ld, Ms.d, ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), B,
                                b.n_users, b.n_items, coef.ptr, ws.ptr, mf.ptr, reg.ptr, flag.data_ptr() + 4 if with_flag else None,
                                _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert Ms.untouched() and Es.untouched()
    f = flag.cpu().numpy()
    assert f[0] == f[2] == SENTINEL and f[1] in (0, 1) and (with_flag or f[1] == 0)
    assert all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(ids, (b.users, b.pos, b.neg)))
    return coef.values()[0], ws.values()[0], mf.values()[0, 0], reg.values()[0, 0], int(f[1])


def run_grad(mode, b, coef, src, out, scale=0.0, zero=None):
    """one call on the Seats src / out / zero; returns out's window (and zero's): guards checked, src whole"""
    lib = _lib.load()
    ids = ids_of(b)
    order = torch.from_numpy(b.order()).to(DEV)
    c = None if coef is None else torch.from_numpy(np.ascontiguousarray(coef, F32)).to(DEV)
    rc = lib.gdmcf_bpr_grad_f32(mode, order.data_ptr(), ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(), b.B, b.n_users,
                                b.n_items, None if c is None else c.data_ptr(), src.ptr, src.ld, src.d, out.ptr, out.ld, scale,
                                None if zero is None else zero.ptr, 0 if zero is None else zero.ld, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert src.untouched() and np.array_equal(order.cpu().numpy(), b.order())
    assert c is None or np.array_equal(c.cpu().numpy(), np.ascontiguousarray(coef, F32))
    return out.values(), None if zero is None else zero.values()


def sentinel_rows(N, d):
    return np.full((N, d), SENTINEL, np.int32).view(F32)


# ---- loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.ALL_WIDTHS)
def test_loss(d):
    """spread, hub_item and bad_ids at B = 1, G + 1 and 128 on the dyadic and the tails table: x is exact, so coef and soft are
    inside the measured TRANS_TOL (coef, soft) of float64, rg and reg bit for bit, mf inside its derived bounds"""
    LG = R.lane_group(d)
    seats, worst = {}, [0.0, 0.0]
    for kind, make in (("dyadic", R.dyadic_table), ("tails", R.tails_table)):
        for b in R.loss_batches(LG):
            if (kind, b.N) not in seats:
                M, E0 = make(b.N, d, 1), R.dyadic_table(b.N, d, 2)
                seats[kind, b.N] = (M, E0, Seat(b.N, d, data=M), Seat(b.N, d, data=E0))
            M, E0, Ms, Es = seats[kind, b.N]
            ref = R.loss_ref(M, E0, b)
            coef, ws, mf, reg, flag = run_loss(Ms, Es, b)
            seen = R.check_loss(coef, ws, mf, reg, ref, d, TRANS_TOL)
            worst = [max(w, s) for w, s in zip(worst, seen)]
            assert flag == ref["flag"] == int(b.name == "bad_ids"), (kind, b.name, b.B)
            if b.name == "hub_item" and kind == "dyadic":
                assert R.same_bits(coef, np.full(b.B, F32(0.5) / F32(b.B), F32))
            if b.name == "bad_ids":
                ok, c = b.ok(), b.clean() if b.ok().any() else None
                got = run_loss(Ms, Es, b, with_flag=False)  # flag = NULL: the same call, nothing raised
                assert all(R.same_bits(x, y) for x, y in zip(got[:4], (coef, ws, mf, reg)))
                if c is not None:  # the good triples as in the batch without the bad ones, but for the / B
                    coef_c, ws_c, _, _, flag_c = run_loss(Ms, Es, c)
                    assert flag_c == 0 and R.same_bits(ws[:b.B][ok], ws_c[:c.B]) and R.same_bits(ws[b.B:][ok], ws_c[c.B:])
                    # sig / B and sig / B_clean, one correctly rounded division each: both within u sig of sig <= e / (1 - u),
                    # wherever the quotients are normal float32 numbers (x above DEEP_X)
                    a, e = coef[ok].astype(np.float64) * b.B, coef_c.astype(np.float64) * c.B
                    normal = ref["x"][ok] >= R.DEEP_X
                    assert (np.abs(a - e)[normal] <= 2 * R.U / (1 - R.U) * e[normal]).all() and normal.sum() > c.B / 2
    print("loss d %3d: max |coef / ref - 1| %.3f u   max |soft / ref - 1| %.3f u   (u = 2^-24)" % (d, worst[0] / R.U, worst[1] / R.U))


@pytest.mark.parametrize("LG", R.LGS)
def test_loss_on_a_real_table(LG):
    """standard normal tables, the widest d of the class: x inside x_bound, carried through |sigmoid'| <= 1 / 4 and
    |softplus'| <= 1; rg and reg inside their relative bounds"""
    d = R.WIDTHS[LG][-1]
    for b in (R.spread(256 // LG + 1), R.spread(128), R.bad_ids(128)):
        M, E0 = R.real_table(b.N, d, 1), R.real_table(b.N, d, 2)
        coef, ws, mf, reg, flag = run_loss(Seat(b.N, d, data=M), Seat(b.N, d, data=E0), b)
        R.check_loss(coef, ws, mf, reg, R.loss_ref(M, E0, b), d, TRANS_TOL, exact_x=False, exact_reg=False)
        assert flag == int(b.name == "bad_ids")


# ---- scatter --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", R.SCATTER_WIDTHS)
def test_scatter_mode0(d):
    """every batch builder; dyadic coefficients on a dyadic table: each written row equals the float64 sum bit for bit, rows of
    no entry (and of out-of-range entries) keep the sentinel; then a real table with the loss kernel's own coef: inside
    scatter_bound -- the one place the two kernels run as a chain"""
    LG = R.lane_group(d)
    for b in R.scatter_batches(LG):
        src = R.dyadic_table(b.N, d, 3)
        coef = np.where(b.ok(), R.dyadic_coef(b.B, 5), 0).astype(F32)  # (a triple with a bad id has coef 0, as the loss kernel gives)
        got, _ = run_grad(0, b, coef, Seat(b.N, d, data=src), Seat(b.N, d, fill=SENTINEL))
        R.check_mode0(got, b, coef, src, sentinel_rows(b.N, d))
        M, E0 = R.real_table(b.N, d, 1), R.real_table(b.N, d, 2)
        Ms = Seat(b.N, d, data=M)
        kcoef = run_loss(Ms, Seat(b.N, d, data=E0), b)[0]
        assert (kcoef[~b.ok()] == 0).all() and (kcoef[b.ok()] >= 0).all()
        got, _ = run_grad(0, b, kcoef, Ms, Seat(b.N, d, fill=SENTINEL))
        R.check_mode0(got, b, kcoef, M, sentinel_rows(b.N, d), exact=False)


@pytest.mark.parametrize("d", R.SCATTER_WIDTHS)
def test_scatter_mode1(d):
    """scale = 2^-7, integer src and out: out += scale * multiplicity * src bit for bit (multiplicities 1, LG, LG + 1, 2 LG and
    2 B occur: tests/test_host_bpr_ref.py); with zero_rows exactly the batch's rows are cleared in columns [0, d)"""
    LG = R.lane_group(d)
    for b in R.scatter_batches(LG):
        src, out0, zero0 = R.int_table(b.N, d, 4), R.int_table(b.N, d, 6, -5, 5), R.int_table(b.N, d, 8, 1, 4)
        Ss = Seat(b.N, d, data=src)
        for with_zero in (False, True):
            out, zero = Seat(b.N, d, data=out0, fill=SENTINEL), Seat(b.N, d, data=zero0, fill=SENTINEL) if with_zero else None
            got, got_zero = run_grad(1, b, None, Ss, out, SCALE, zero)
            R.check_mode1(got, got_zero, b, src, out0, SCALE, zero0 if with_zero else None)
            if with_zero:
                assert np.array_equal((got_zero == 0).all(1), b.multiplicity() > 0)


# ---- strides and alignment ------------------------------------------------------------------------------------------------------
LAYOUTS = {"ld_d_plus_4": lambda d: (d + 4, 0), "ld_d_plus_1": lambda d: (d + 1, 0), "four_bytes_off": lambda d: (d, 1)}


@pytest.mark.parametrize("which", ["all", "M", "E0", "out", "zero_rows"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("d", [64, 260])
def test_strides_and_alignment(d, layout, which):
    """`multiples`: the named operand (or all of them) in the given layout, the others contiguous and aligned -- every result has
    the bits of the all-contiguous call (one summation order in the float4 and the element-wise instantiation)"""
    LG, (ld, off) = R.lane_group(d), LAYOUTS[layout](d)
    b = R.multiples(LG)
    M, E0, coef = R.dyadic_table(b.N, d, 1), R.int_table(b.N, d, 2), R.dyadic_coef(b.B, 5)
    out0, zero0 = R.int_table(b.N, d, 6, -5, 5), R.int_table(b.N, d, 8, 1, 4)

    def seat(name, data, fill=NAN_BITS, plain=False):
        moved = not plain and which in ("all", name)
        s = Seat(b.N, d, ld if moved else d, off if moved else 0, data=data, fill=fill)
        assert (s.ptr % 16 == 0 and s.ld % 4 == 0) == (not moved or layout == "ld_d_plus_4")
        return s

    def results(plain):
        Ms, Es = seat("M", M, plain=plain), seat("E0", E0, plain=plain)
        loss = run_loss(Ms, Es, b)[:4]
        g0, _ = run_grad(0, b, coef, Ms, seat("out", None, SENTINEL, plain))
        g1, z1 = run_grad(1, b, None, Es, seat("out", out0, SENTINEL, plain), SCALE, seat("zero_rows", zero0, SENTINEL, plain))
        g2, _ = run_grad(1, b, None, Es, seat("out", out0, SENTINEL, plain), SCALE)
        return (*loss, g0, g1, z1, g2)

    want, got = results(True), results(False)
    for i, (w, g) in enumerate(zip(want, got)):
        assert R.same_bits(w, g), i
    R.check_mode0(got[4], b, coef, M, sentinel_rows(b.N, d))
    R.check_mode1(got[5], got[6], b, E0, out0, SCALE, zero0)


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 129, 260])
def test_two_launches_give_the_same_bits(d):
    """hub_item on a real table: one run of 2 B entries, summed in one order"""
    b = R.hub_item(130)
    M, E0 = R.real_table(b.N, d, 1), R.real_table(b.N, d, 2)
    Ms, Es = Seat(b.N, d, data=M), Seat(b.N, d, data=E0)
    coef = R.real_table(1, b.B, 9)[0]
    first = None
    for _ in range(2):
        out = (*run_loss(Ms, Es, b)[:4], run_grad(0, b, coef, Ms, Seat(b.N, d, fill=SENTINEL))[0],
               *run_grad(1, b, None, Es, Seat(b.N, d, data=M, fill=SENTINEL), 0.37, Seat(b.N, d, data=E0, fill=SENTINEL)))
        if first is None:
            first = out
        assert all(R.same_bits(x, y) for x, y in zip(first, out))
    R.check_mode0(first[4], b, coef, M, sentinel_rows(b.N, d), exact=False)
