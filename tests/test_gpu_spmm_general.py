"""GPU (-m gpu): the three SpMM generations (csrc/spmm_csr.hip, csrc/spmm_bundle.hip) on general CSR matrices, against the float64
model of tests/spmm_ref.py: rectangular matrices with signed values, stored zeros and empty rows, every degree boundary of the
schedules (the matrices `edges` and `bulk`; tests/test_host_spmm_general.py proves that they hit them), row strides wider than
d, up to 8 addends, any scale, and gathered tables on both sides of 4 GiB.

No tolerance is measured: integer-valued data is exact in float32 in any summation order and must match bit for bit; real data
must lie inside the derived rounding bound.  Every operand is a column slice of a wider buffer full of NaN: whatever the kernels
write outside Y[:n_rows, :d], or read outside their operands, shows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib
from gdmcf_amd.spmm_schedule import SpmmSchedule, spmm_plan
from tests import spmm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GENS = ("1", "2", "3")
WIDTHS = (8, 16, 32, 64, 128, 256)
LEAD = 4  # floats in front of every operand's first row: 16 bytes, the operand stays aligned


@functools.lru_cache(maxsize=None)
def matrix(name):
    return getattr(R, name)()


@functools.lru_cache(maxsize=None)
def operands(name, mode, d):
    """(vals, X, the 8 addends) of a case, read-only; row 0 of X is NaN where no entry of the matrix names column 0."""
    ip, ix, n_cols = matrix(name)
    vals, X, adds = R.data(mode, len(ix), len(ip) - 1, n_cols, d, seed=1)
    if name == "edges":
        X[0] = np.nan
    for a in [X] + adds:
        a.setflags(write=False)
    return vals, X, tuple(adds)


@functools.lru_cache(maxsize=None)
def expected(name, mode, d, n_add, scale):
    """(float64 reference, bound), computed once per case and shared by the generations."""
    ip, ix, _ = matrix(name)
    vals, X, adds = operands(name, mode, d)
    ref = R.reference(ip, ix, vals, X, adds[:n_add], scale)
    bnd = R.bound(ip, ix, vals, X, adds[:n_add], scale)
    ref.setflags(write=False)
    bnd.setflags(write=False)
    return ref, bnd


@functools.lru_cache(maxsize=None)
def schedule(name, mode, gen, d):
    ip, ix, n_cols = matrix(name)
    return SpmmSchedule(ip, ix, operands(name, mode, d)[0], n_cols, d, gen, None, DEV)


class Padded:
    """A [rows, d] float32 operand inside a flat device buffer full of NaN: `lead` floats, then rows of stride ld (the last one
    whole), then 4 more floats.  `t` is the operand."""

    def __init__(self, rows, d, ld, values=None, lead=LEAD):
        self.rows, self.d, self.ld, self.lead = rows, d, ld, lead
        self.flat = torch.full((lead + rows * ld + 4,), float("nan"), dtype=torch.float32, device=DEV)
        self.t = torch.as_strided(self.flat, (rows, d), (ld, 1), lead)
        if values is not None:
            self.t.copy_(torch.tensor(values))
        self.before = self.flat.clone()

    def bits(self):
        return self.flat.view(torch.int32)

    def assert_unchanged(self, what):
        assert torch.equal(self.bits(), self.before.view(torch.int32)), f"{what} was written"

    def assert_only_written(self, rows, what):
        """Everything but t[:rows] is still NaN."""
        rest = self.flat.clone()
        torch.as_strided(rest, (rows, self.d), (self.ld, 1), self.lead).fill_(float("nan"))
        assert bool(torch.isnan(rest).all()), f"{what}: written outside [:{rows}, :{self.d}]"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run_case(name, mode, gen, d, n_add, scale, launch=None, ldx=None, ldy=None, ld_add=None, x_lead=LEAD, add_lead=LEAD):
    """One product through SpmmSchedule.launch -- or through launch_, partial = launch(X, Y, adds) -- with padded, NaN-surrounded
    operands, twice; checks everything but the values: the result is returned as a host array [n_rows, d]."""
    ip, ix, n_cols = matrix(name)
    n_rows = len(ip) - 1
    vals, Xh, addh = operands(name, mode, d)
    X = Padded(n_cols, d, ldx or d + 4, Xh, lead=x_lead)
    Y = Padded(n_rows + 3, d, ldy or d + 8)
    adds = [Padded(n_rows, d, ld_add or d + 12, a, lead=add_lead) for a in addh[:n_add]]
    if launch is None:
        sched = schedule(name, mode, gen, d)
        partial = sched.partial

        def launch():
            sched.launch(X.t, n_rows, n_cols, Y.t, [a.t for a in adds], scale, 0.0, _lib.stream_ptr())
    else:
        launch, partial = launch(X, Y, adds)
    out = []
    for _ in range(2):
        partial.fill_(float("nan"))  # the result must not depend on what the partial sums held before
        Y.flat.fill_(float("nan"))
        launch()
        torch.cuda.synchronize()
        out.append(Y.t[:n_rows].cpu().numpy())
        Y.assert_only_written(n_rows, f"Y ({name}, generation {gen}, d {d})")
        X.assert_unchanged("X")
        for a in adds:
            a.assert_unchanged("an addend")
    assert np.isfinite(out[0]).all(), "a non-finite output: something that no stored entry names was gathered"
    assert np.array_equal(bits(out[0]), bits(out[1])), "two launches of one schedule differ"
    return out[0]


def assert_exact(got, ref, what):
    want = ref.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref)  # the reference is a float32 number
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} elements differ from the exact product, first at row {bad[0][0]} column {bad[0][1]}: "
                           f"{got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}; rows {np.unique(bad[:, 0])[:12]}")


# ---- a. exact product ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_add", [0, 1, 8])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "bulk"])
@pytest.mark.parametrize("gen", GENS)
def test_exact_product(gen, name, d, n_add):
    """Integer-valued data: bit-for-bit the float64 product, with ldx = d + 4, ldy = d + 8, ld_add = d + 12, NaN around every
    operand, behind Y's rows and in the partial sums, and NaN in the row of X that no entry gathers."""
    scale = R.int_scale(int(gen), d // 8, n_add)
    got = run_case(name, "int", gen, d, n_add, scale)
    assert_exact(got, expected(name, "int", d, n_add, scale)[0], f"generation {gen}, {name}, d {d}, {n_add} addends, scale {scale}")


# ---- b. real values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_add", [0, 3])
@pytest.mark.parametrize("d", [8, 64, 256])
@pytest.mark.parametrize("name", ["edges", "bulk"])
def test_real_values_lie_inside_the_rounding_bound(name, d, n_add):
    """Signed normal data: every element of every generation within the derived bound of the float64 product (any summation
    order, with or without FMA), and the generations pairwise within the sum of their bounds."""
    scale = float(np.float32((0.37, -1.0 / 3.0)[n_add > 0]))  # the float32 number the kernels are handed
    ref, bnd = expected(name, "real", d, n_add, scale)
    got = {gen: run_case(name, "real", gen, d, n_add, scale).astype(np.float64) for gen in GENS}
    for gen in GENS:
        err = np.abs(got[gen] - ref)
        worst = np.unravel_index(np.argmax(err - bnd), err.shape)
        print(f"generation {gen} {name} d {d} n_add {n_add}: max error {err.max():.3e}, bound there "
              f"{bnd[np.unravel_index(np.argmax(err), err.shape)]:.3e}")
        assert (err <= bnd).all(), f"generation {gen}: row {worst[0]} column {worst[1]} is off by {err[worst]:.3e}, bound {bnd[worst]:.3e}"
    for a, b in (("1", "2"), ("1", "3"), ("2", "3")):
        assert (np.abs(got[a] - got[b]) <= 2 * bnd).all(), f"generations {a} and {b} disagree"


# ---- c. the generic kernel, through the C entry ----------------------------------------------------------------------------
def csr_entry_launcher(name, mode, d, n_add, scale):
    """run_case's `launch` for gdmcf_spmm_csr_f32 with a plan without short rows (spmm_plan(short=-1))."""
    ip, ix, _ = matrix(name)
    n_rows = len(ip) - 1
    pl = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in spmm_plan(ip, short=-1, d=d).items()}
    assert pl["n_short"] == 0 and int(np.diff(pl["lptr"].cpu().numpy()).max()) == 18
    col, val = torch.from_numpy(ix).to(DEV), torch.from_numpy(operands(name, mode, d)[0]).to(DEV)
    partial = torch.empty(max(pl["n_slots"], 1), d, dtype=torch.float32, device=DEV)

    def make(X, Y, adds):
        arr = (ctypes.c_void_p * max(n_add, 1))(*[a.t.data_ptr() for a in adds])

        def launch():
            _lib.check(_lib.load().gdmcf_spmm_csr_f32(
                pl["vbeg"].data_ptr(), pl["vend"].data_ptr(), pl["vrow"].data_ptr(), pl["vslot"].data_ptr(), pl["vrow"].numel(), 0,
                pl["lrow"].data_ptr(), pl["lptr"].data_ptr(), pl["lrow"].numel(), col.data_ptr(), val.data_ptr(), n_rows,
                X.t.data_ptr(), X.ld, d, Y.t.data_ptr(), Y.ld, partial.data_ptr(), arr, n_add, adds[0].ld if adds else X.ld,
                scale, 0.0, _lib.stream_ptr()))
        return launch, partial
    return make


GENERIC = [(d, {}) for d in (1, 3, 7, 20, 100, 260, 512)] + [
    (64, dict(x_lead=LEAD + 1)),  # X offset by one float
    (64, dict(ldy=65)),           # ldy = d + 1
    (64, dict(add_lead=LEAD + 1)),  # an addend offset by one float
]


@pytest.mark.parametrize("d,layout", GENERIC, ids=[f"{d}-{'-'.join(k) or 'plain'}" for d, k in GENERIC])
def test_generic_kernel_exact(d, layout):
    """spmm_generic_kernel + spmm_combine_kernel (18 slots in one row): widths that are no power-of-two number of 16-byte
    lanes, and d = 64 with a misaligned X, Y row stride or addend.  Integer-valued data, exact; two addends."""
    n_add = 2
    scale = R.int_scale(d)
    got = run_case("edges", "int", "1", d, n_add, scale, launch=csr_entry_launcher("edges", "int", d, n_add, scale), **layout)
    assert_exact(got, expected("edges", "int", d, n_add, scale)[0], f"generic kernel, d {d}, {layout}")


# ---- d. refusals -----------------------------------------------------------------------------------------------------------
def refused(gen, exc, match, d=64, n_add=1, x_lead=LEAD, ld_add=None):
    """The launch raises `exc` out of _lib.check (its text is the C entry's) and leaves the NaN-filled Y as it was."""
    name = "edges"
    ip, ix, n_cols = matrix(name)
    n_rows = len(ip) - 1
    _, Xh, addh = operands(name, "int", d)
    X = Padded(n_cols, d, d + 4, Xh, lead=x_lead)
    Y = Padded(n_rows + 3, d, d + 8)
    if ld_add is None:
        adds = [Padded(n_rows, d, d + 12, addh[k % len(addh)]).t for k in range(n_add)]
    else:  # rows that overlap: a row stride below d
        adds = [torch.as_strided(torch.zeros(n_rows * d, device=DEV), (n_rows, d), (ld_add, 1)) for _ in range(n_add)]
    sched = schedule(name, "int", gen, d)
    with pytest.raises(exc, match=match):
        sched.launch(X.t, n_rows, n_cols, Y.t, adds, 1.0, 0.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    Y.assert_unchanged("Y")


@pytest.mark.parametrize("gen", ["2", "3"])
def test_bundled_and_streamed_refuse_a_misaligned_table(gen):
    refused(gen, NotImplementedError, "16-byte aligned rows", x_lead=LEAD + 1)


def test_first_generation_refuses_short_rows_on_a_misaligned_table():
    assert schedule("edges", "int", "1", 64).plan["n_short"] > 0
    refused("1", ValueError, "short-row path", x_lead=LEAD + 1)


@pytest.mark.parametrize("gen", GENS)
def test_nine_addends_are_refused(gen):
    refused(gen, ValueError, "bad addends", n_add=9)


@pytest.mark.parametrize("gen", GENS)
def test_an_addend_stride_below_d_is_refused(gen):
    refused(gen, ValueError, "bad addends", ld_add=60)


# ---- e. the 4 GiB boundary -------------------------------------------------------------------------------------------------
BIG_LD = 1 << 18  # floats: 1 MiB a row


@pytest.fixture(scope="module")
def big_tables():
    """Hands the 4 GiB blocks back to the device once the cases below are through."""
    yield
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [4095, 4096, 4097])
@pytest.mark.parametrize("gen", GENS)
def test_table_at_the_4gib_boundary(gen, n, big_tables):
    """d = 64 columns of an [n, 2^18] float32 view (1 MiB a row; only those columns are ever written), 200 rows that all gather
    row n - 1.  n = 4095: the table ends below 2^32 bytes, generations 2 and 3 form 32-bit offsets, beyond 2^31 for the upper
    half of the rows.  n = 4096: exactly 2^32 bytes, the WIDE instantiations run (every offset still fits 32 bits, so this case
    alone would not notice 32-bit offsets in their place).  n = 4097: row 4096 lies at byte 2^32, where a 32-bit offset wraps to
    row 0 -- inside the buffer, a wrong value and no fault.  Integer-valued data, exact."""
    d = 64
    ip, ix = R.boundary_matrix(n)
    n_rows = len(ip) - 1
    assert ix.max() == n - 1 and (ix[ip[1:] - 1] == n - 1).all() and (ix >= 2048).any()
    vals, Xh, addh = R.data("int", len(ix), n_rows, n, d, seed=3, n_add=1)
    scale = R.int_scale(int(gen), n)
    buf = torch.empty(max(n, 4096) * BIG_LD, dtype=torch.float32, device=DEV)  # no skip: an allocation failure is a failure
    X = buf.view(-1, BIG_LD)[:n, :d]
    assert X.stride(0) == BIG_LD and (n * BIG_LD * 4 >= 1 << 32) == (n >= 4096)
    X.copy_(torch.tensor(Xh))
    add = torch.tensor(addh[0], device=DEV)
    Y = torch.full((n_rows, d), float("nan"), dtype=torch.float32, device=DEV)
    sched = SpmmSchedule(ip, ix, vals, n, d, gen, None, DEV)
    sched.partial.fill_(float("nan"))
    sched.launch(X, n_rows, n, Y, [add], scale, 0.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    got = Y.cpu().numpy()
    del buf, X
    assert_exact(got, R.reference(ip, ix, vals, Xh, addh, scale), f"generation {gen}, table of {n} MiB")
