"""CPU (-m "not gpu"): the host side of the general SpMM tests (tests/spmm_ref.py, tests/test_gpu_spmm_general.py).  The test
matrices must produce the schedule features they were built for, with the knobs' defaults; the "int" value mode must stay exact in
float32; the error bound must hold for float32 evaluations in several orders; the third generation's packed stream must reproduce
the product on both matrices; and SpmmSchedule.launch must refuse what the C entries cannot see."""
import numpy as np
import pytest
import torch

from gdmcf_amd import spmm_schedule as S
from tests import spmm_ref as R

WIDTHS = (8, 64, 256)
ALL_WIDTHS = (8, 16, 32, 64, 128, 256)
GENERIC_WIDTHS = (1, 3, 7, 20, 100, 260, 512)
BOUNDARY_N = (4095, 4096, 4097)


def test_the_knobs_are_at_the_defaults_the_matrices_were_built_for():
    assert (S.SPMM_SHORT, S.SPMM_CHUNK, S.SPMM_SMAX, S.SPMM_PIECE) == (48, 256, 64, 128)


def test_edges_and_bulk_are_what_they_claim():
    ip, ix, n_cols = R.edges()
    deg = np.diff(ip)
    assert tuple(deg) == R.EDGES_DEGREES and n_cols == R.EDGES_COLS == 4608 and len(ix) == ip[-1]
    assert ix.min() == 1 and ix.max() == n_cols - 1  # column 0 never, the last column referenced
    for r in np.nonzero(deg)[0]:
        row = ix[ip[r]:ip[r + 1]]
        assert (np.diff(row) > 0).all() and r in row  # sorted, unique, diagonal entry
    ip, ix, n_cols = R.bulk()
    deg = np.diff(ip)
    assert (len(deg), n_cols) == (2000, 700) and deg.max() == 70 and deg[0] == 0 and deg[-1] == 0
    assert 0.07 < (deg == 0).mean() < 0.14
    assert ix.min() >= 0 and ix.max() < n_cols
    assert all((np.diff(ix[ip[r]:ip[r + 1]]) > 0).all() for r in range(len(deg)))
    for mode in ("int", "real"):
        vals = R.data(mode, int(ip[-1]), len(deg), n_cols, 8, seed=0, n_add=0)[0]
        assert (vals == 0).sum() >= 3 and (vals < 0).any() and (vals > 0).any()  # stored zeros, signed values


@pytest.mark.parametrize("d", WIDTHS)
def test_edges_first_generation_plan(d):
    """18 short rows (empty ones among them), 6 cut rows, one of 18 partial slots (spmm_combine_kernel's 16-slot loop runs and
    leaves a remainder), pieces of exactly SPMM_CHUNK and one nonzero, rows on both sides of SPMM_SHORT."""
    ip, ix, n_cols = R.edges()
    deg = np.diff(ip)
    pl = S.spmm_plan(ip, d=d)
    ns = pl["n_short"]
    assert ns == 18 > 0 and (deg[pl["vrow"][:ns]] == 0).any() and deg[pl["vrow"][:ns]].max() == S.SPMM_SHORT
    ln = (pl["vend"] - pl["vbeg"])[ns:]
    assert ln.max() == S.SPMM_CHUNK > 64 and ln.min() == 1 and S.SPMM_SHORT + 1 in ln
    slots = np.diff(pl["lptr"])
    assert len(pl["lrow"]) == 6 > 0 and slots.max() == 18 >= 17 and slots.min() == 2
    NPAR = 64 // (d // 4)  # spmm_vec_kernel: the unrolled loop takes 4 * NPAR nonzeros a trip, the tail NPAR
    assert (ln >= 4 * NPAR).any() and (ln % (4 * NPAR) != 0).any() and (ln < 4 * NPAR).any()
    assert NPAR == 1 or ((ln % NPAR != 0).any() and (ln < NPAR).any())  # lane groups without a nonzero in the last trip


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("gen", ["2", "3"])
def test_edges_bundled_and_streamed_plan(gen, d):
    """Bundled rows on both sides of SPMM_SMAX, pieces of SPMM_PIECE - 1, SPMM_PIECE and (SPMM_PIECE + 1) cut in two, pieces
    with a second 64-entry batch, rows cut at column ranges, a cut row of at least 17 slots (spmm_bundle_combine_kernel's
    4 * G loop runs with a remainder from d = 32 on), several bundles at d = 256, empty rows inside bundles."""
    ip, ix, n_cols = R.edges()
    deg = np.diff(ip)
    pl = S.spmm_bundle_plan(ip, ix, d=d, n_cols=n_cols)
    G = pl["G"]
    n_short = int((pl["srow"] >= 0).sum())
    assert n_short == 21 > 0 and pl["slen"].max() == S.SPMM_SMAX and deg[pl["lrow"]].min() == S.SPMM_SMAX + 1
    assert pl["n_bundles"] >= -(-21 // G)
    if d == 256:
        assert pl["n_bundles"] > 1
    llen = pl["llen"]
    assert llen.max() == S.SPMM_PIECE > 64 and S.SPMM_PIECE - 1 in llen
    assert sorted(llen[pl["lrow"] == 21]) == [64, 65]  # the row of SPMM_PIECE + 1 nonzeros, inside one column range
    slots = np.diff(pl["cptr"])
    assert len(pl["crow"]) > 0 and slots.max() >= 17
    for r, n in zip(pl["crow"], slots):  # a cut never needed by SPMM_PIECE alone: a column-range cut
        if n > -(-deg[r] // S.SPMM_PIECE):
            break
    else:
        raise AssertionError("no row is cut at a column range")
    if G <= 8:  # the unrolled loop of the combine takes 4 * G slots a trip: it runs, and leaves a remainder, from d = 32 on
        assert any(n > 3 * G and n % (4 * G) != 0 for n in slots)  # (d = 8, 16: a row of 4400 has too few pieces for a trip)
    # an empty row shares a bundle with a non-empty one (G > 1), or is a bundle of its own (G = 1)
    srow, slen = pl["srow"].reshape(-1, G), pl["slen"].reshape(-1, G)
    assert (((srow >= 0) & (slen == 0)).any(1) & ((slen > 0).any(1) | (G == 1))).any()
    assert G == 1 or (srow < 0).any()  # 21 rows: some bundle is padded
    if gen == "3":
        vals = R.data("int", len(ix), len(deg), n_cols, d, seed=1, n_add=0)[0]
        pk = S.spmm_stream_pack(pl, ip, ix, vals, d=d)
        ud = pk["ud"].reshape(-1, pk["DW"])
        bundles = ud[ud[:, 0] >= 0][:, 1:1 + G]
        assert ((bundles >= 0) & (bundles & (1 << 30) != 0)).any()  # the empty-row flag is in use


@pytest.mark.parametrize("d", WIDTHS)
def test_bulk_plans(d):
    """bulk: bundles whose rows have one length and bundles whose rows differ, empty rows inside bundles with gathered rows,
    rows above SPMM_SMAX, many waves; the first generation runs it through the short-row kernel but for its 120 longest rows."""
    ip, ix, n_cols = R.bulk()
    deg = np.diff(ip)
    p1 = S.spmm_plan(ip, d=d)
    assert p1["n_short"] == int((deg <= S.SPMM_SHORT).sum()) > 1000 and len(p1["vrow"]) > p1["n_short"]
    pl = S.spmm_bundle_plan(ip, ix, d=d, n_cols=n_cols)
    G = pl["G"]
    srow, slen = pl["srow"].reshape(-1, G), pl["slen"].reshape(-1, G)
    real = srow >= 0
    assert pl["n_bundles"] > 1 and pl["n_waves"] > 32 and pl["n_pieces"] > 0 and len(pl["crow"]) > 0
    if G > 1:
        lo = np.where(real, slen, 1 << 20).min(1)
        hi = np.where(real, slen, -1).max(1)
        full = real.all(1)
        assert (full & (lo == hi) & (hi > 0)).any() and (full & (lo != hi)).any()  # equal and unequal lengths
        assert ((lo == 0) & (hi > 0)).any()  # an empty row beside gathered ones
    else:
        assert (slen == 0).any()


def _int_cases():
    """(name, indptr, indices, n_rows, n_cols, d) of every "int" case that runs on the GPU."""
    for name in ("edges", "bulk"):
        ip, ix, n_cols = getattr(R, name)()
        for d in ALL_WIDTHS + (GENERIC_WIDTHS if name == "edges" else ()):
            yield name, ip, ix, len(ip) - 1, n_cols, d
    for n in BOUNDARY_N:
        ip, ix = R.boundary_matrix(n)
        yield f"boundary{n}", ip, ix, len(ip) - 1, n, 64


def test_int_mode_is_exact_in_float32():
    """Every partial sum of every "int" case, in any order, is bounded by sum |a||x| + sum |addend| < 2^24, and the scales are
    powers of two: the float64 reference is a float32 number and any float32 evaluation must reproduce it bit for bit."""
    assert R.INT_VAL_MAX * R.INT_X_MAX * max(R.EDGES_DEGREES) + R.N_ADD_MAX * R.INT_X_MAX == 4400 * 16 + 64 < 2 ** 24
    for name, ip, ix, n_rows, n_cols, d in _int_cases():
        vals, X, adds = R.data("int", len(ix), n_rows, n_cols, d, seed=1)
        assert np.abs(vals).max() <= R.INT_VAL_MAX and np.abs(X).max() <= R.INT_X_MAX
        assert R.magnitude(ip, ix, vals, X, adds).max() < 2 ** 24, name
        for scale in R.INT_SCALES:
            ref = R.reference(ip, ix, vals, X, adds, scale)
            assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), (name, d, scale)
            assert np.array_equal(ref / scale, np.rint(ref / scale))
    assert {R.int_scale(k) for k in range(3)} == set(R.INT_SCALES)


def _f32_eval(ip, ix, vals, X, adds, scale, order):
    """(A X + addends) * scale with every operation rounded to float32, the terms of a row added in `order`."""
    n, d = len(ip) - 1, X.shape[1]
    Y = np.zeros((n, d), dtype=np.float32)
    for r in range(n):
        terms = list(vals[ip[r]:ip[r + 1], None] * X[ix[ip[r]:ip[r + 1]]]) + [a[r] for a in adds]  # float32 products
        if order == "reversed":
            terms = terms[::-1]
        if order == "pairwise":
            while len(terms) > 1:
                terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
            acc = terms[0] if terms else np.zeros(d, np.float32)
        else:
            acc = np.zeros(d, np.float32)
            for t in terms:
                acc = acc + t
        assert acc.dtype == np.float32
        Y[r] = acc * np.float32(scale)
    return Y


@pytest.mark.parametrize("order", ["forward", "reversed", "pairwise"])
def test_bound_holds_for_float32_evaluations(order):
    """The derived bound against real float32 arithmetic, on the rows of `edges` (degrees 0 .. 4400) with signed normal data."""
    ip, ix, n_cols = R.edges()
    n_rows, d = len(ip) - 1, 8
    vals, X, adds = R.data("real", len(ix), n_rows, n_cols, d, seed=2, n_add=3)
    X[0] = np.nan
    for use, scale in ((adds, 0.25), ([], -1.7)):
        ref = R.reference(ip, ix, vals, X, use, scale)
        bnd = R.bound(ip, ix, vals, X, use, scale)
        err = np.abs(_f32_eval(ip, ix, vals, X, use, scale, order).astype(np.float64) - ref)
        assert np.isfinite(ref).all() and (err <= bnd).all()
        assert (bnd[np.diff(ip) == 0] == 0).all() or use  # an empty row without addends is exactly zero


def test_reference_reads_stored_entries_only_and_sums_onto_plus_zero():
    ip, ix = np.array([0, 2, 2, 3]), np.array([1, 2, 1], dtype=np.int32)
    vals = np.array([0.0, 0.0, -2.0], dtype=np.float32)
    X = np.array([[np.nan], [-3.0], [5.0]], dtype=np.float32)
    ref = R.reference(ip, ix, vals, X, [], -0.5)
    assert np.array_equal(ref, [[0.0], [0.0], [-3.0]])
    assert np.signbit(ref[:2]).all()  # (+0 + 0 * -3 + 0 * 5) * -0.5 = -0, as in the kernels; the empty row likewise
    assert np.array_equal(R.bound(ip, ix, vals, X, [], -0.5)[:2], [[0.0], [0.0]])


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "bulk"])
def test_stream_pack_emulation_reproduces_the_product(name, d):
    ip, ix, n_cols = getattr(R, name)()
    n_rows = len(ip) - 1
    vals, X, _ = R.data("int", len(ix), n_rows, n_cols, d, seed=1, n_add=0)
    X[0] = np.nan  # edges: nobody gathers column 0, not even the padding of a unit
    if name == "bulk":
        X[0] = 1.0
    pk = S.spmm_stream_pack(S.spmm_bundle_plan(ip, ix, d=d, n_cols=n_cols), ip, ix, vals, d=d)
    Y = R.emulate(n_rows, X, d, pk)
    assert np.array_equal(Y, R.reference(ip, ix, vals, X))  # integers: exact


# ---- SpmmSchedule.launch refuses what the C entries cannot see (before anything is loaded or launched) ---------------------
def _sched_and_args():
    ip, ix = np.array([0, 2, 3, 3]), np.array([0, 3, 1], dtype=np.int32)
    sched = S.SpmmSchedule(ip, ix, np.ones(3, np.float32), 4, 8, "1", None, "cpu")
    return sched, dict(X=torch.zeros(4, 8), out=torch.zeros(3, 8), addends=[torch.zeros(3, 8), torch.zeros(3, 8)])


def _launch(sched, a, n_rows=3, n_x_rows=4):
    return sched.launch(a["X"], n_rows, n_x_rows, a["out"], a["addends"], 1.0, 0.0, None)


@pytest.mark.parametrize("what,change", [
    ("share one row stride", lambda a: a.update(addends=[a["addends"][0], torch.zeros(3, 12)[:, :8]])),
    ("X must be 2-D with unit inner stride", lambda a: a.update(X=torch.zeros(8, 4).t())),
    ("out must be 2-D with unit inner stride", lambda a: a.update(out=torch.zeros(8, 3).t())),
    ("addend 1 must be 2-D with unit inner stride", lambda a: a.update(addends=[a["addends"][0], torch.zeros(8, 3).t()])),
    ("X must be 2-D", lambda a: a.update(X=torch.zeros(32))),
    ("X must be float32", lambda a: a.update(X=torch.zeros(4, 8, dtype=torch.float64))),
    ("out must be float32", lambda a: a.update(out=torch.zeros(3, 8, dtype=torch.bfloat16))),
    ("addend 0 must be float32", lambda a: a.update(addends=[torch.zeros(3, 8, dtype=torch.float16)])),
    ("X has 3 rows", lambda a: a.update(X=torch.zeros(3, 8))),
    ("out has 2 rows", lambda a: a.update(out=torch.zeros(2, 8))),
])
def test_launch_refuses_what_the_c_entry_cannot_see(what, change, monkeypatch):
    from gdmcf_amd import _lib

    def no_load():
        raise AssertionError("the arguments must be checked before the library is loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    sched, args = _sched_and_args()
    change(args)
    with pytest.raises(ValueError, match=what):
        _launch(sched, args)
