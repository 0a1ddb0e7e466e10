"""Host model of the fused LightGCN SpMM, Y = (A X + sum_k addend_k) * scale over the STORED entries of a CSR matrix, with the
test matrices and data that tests/test_host_spmm_general.py and tests/test_gpu_spmm_general.py share -- numpy only, no GPU, no
gdmcf_amd import.

  reference / bound   the product in float64, and how far a float32 evaluation may be from it in ANY summation order
  edges / bulk        two rectangular CSR matrices (sorted, unique columns per row) built to hit the degree boundaries of the
                      three kernel generations (gdmcf_amd/spmm_schedule.py) on purpose
  data                the operands of a case in one of two value modes: "int" (float32 is exact in any order: the result
                      must equal the reference bit for bit) and "real" (signed normals: the result must lie inside `bound`)
  boundary_matrix     the matrix of the 4 GiB table cases
  emulate             spmm_stream_pack's output walked in numpy the way spmm_stream_kernel walks it
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
N_ADD_MAX = 8
EDGES_DEGREES = (0, 0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512,
                 513, 1000, 4400, 0, 7, 0)
EDGES_COLS = 4608
BULK_ROWS, BULK_COLS, BULK_MAX_DEGREE = 2000, 700, 70
INT_SCALES = (1.0, 0.25, -0.5)
INT_VAL_MAX, INT_X_MAX = 2, 8  # "int" mode: |vals| <= 2, |X| and |addends| <= 8


def _rows_sum(indptr, terms):
    """[n_rows, d] sums of the [nnz, d] `terms` over the rows of indptr, each accumulated onto +0.0 (as the kernels do: a row of
    nothing but -0.0 products still sums to +0.0)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    out = np.zeros((len(indptr) - 1, terms.shape[1]), dtype=np.float64)
    full = np.nonzero(np.diff(indptr) > 0)[0]
    if len(full):  # consecutive non-empty rows are adjacent in `terms`: reduceat's segments are exactly the rows
        out[full] = 0.0 + np.add.reduceat(terms, indptr[full], axis=0)
    return out


def reference(indptr, indices, vals, X, addends=(), scale=1.0):
    """float64 Y = (A X + sum of addends) * scale; only the stored entries of A are read (rows of X that no entry names may
    hold anything, NaN included)."""
    X = np.asarray(X)
    Y = _rows_sum(indptr, np.asarray(vals, dtype=np.float64)[:, None] * X[np.asarray(indices)].astype(np.float64))
    for a in addends:
        Y = Y + np.asarray(a, dtype=np.float64)
    return Y * float(scale)


def magnitude(indptr, indices, vals, X, addends=()):
    """sum_j |a_rj| |x_jc| + sum_k |addend_k[r, c]| in float64: what every partial sum of element (r, c) is bounded by."""
    X = np.asarray(X)
    S = _rows_sum(indptr, np.abs(np.asarray(vals, dtype=np.float64))[:, None] * np.abs(X[np.asarray(indices)].astype(np.float64)))
    for a in addends:
        S = S + np.abs(np.asarray(a, dtype=np.float64))
    return S


def bound(indptr, indices, vals, X, addends=(), scale=1.0):
    """Per-element bound on |float32 result - reference| for a float32 evaluation in any summation order, with or without FMA.
    Element (r, c) is reached through at most k = deg_r + n_add + 2 roundings on any path from an input to the result (one per
    product, fewer than deg_r + n_add additions, one for the scale, one to spare), so the standard bound
    gamma_k = k u / (1 - k u) applies to the sum of the magnitudes of its terms."""
    k = (np.diff(np.asarray(indptr, dtype=np.int64)) + len(addends) + 2).astype(np.float64)
    gamma = k * U / (1.0 - k * U)
    return gamma[:, None] * abs(float(scale)) * magnitude(indptr, indices, vals, X, addends)


# ---- the matrices ---------------------------------------------------------------------------------------------------------
def _csr(deg, n_cols, rng, first_col=0, forced=None, window=None):
    """(indptr, indices) with deg[r] sorted unique columns in row r: the columns of forced(r), the others drawn from window(r) =
    (lo, hi), by default from [first_col, n_cols)."""
    rows = []
    for r, k in enumerate(deg):
        must = np.unique(np.asarray(forced(r) if (forced and k) else [], dtype=np.int64))[:k]
        lo, hi = (window(r) if window else None) or (first_col, n_cols)
        pool = np.setdiff1d(np.arange(lo, hi), must)
        rows.append(np.sort(np.concatenate([must, rng.choice(pool, int(k) - len(must), replace=False)])))
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    indices = (np.concatenate(rows) if indptr[-1] else np.zeros(0)).astype(np.int32)
    return indptr, indices


def edges():
    """33 x 4608, one row per degree of EDGES_DEGREES: every threshold of the three schedules, one below, at and one above
    (first generation: SPMM_SHORT 48, SPMM_CHUNK 256, the 4 x NPAR unrolled loop and its tail, a row of 18 partial slots for
    the 16-slot loop of the combine; second and third: SPMM_SMAX 64, SPMM_PIECE 128, the second 64-entry batch of a piece,
    rows cut at column ranges), empty rows at both ends and inside.  Column 0 is never referenced, the last column is (by rows
    of degree 2, 47, 256 and 4400), and every non-empty row holds its diagonal entry.  The rows of degree 127, 128 and 129 keep
    to the first columns, inside one column range of spmm_bundle_plan, so that they stay pieces of 127, 128 and 65 + 64.
    Returns (indptr, indices, n_cols)."""
    rng = np.random.default_rng(4608)
    last = EDGES_COLS - 1
    indptr, indices = _csr(np.array(EDGES_DEGREES), EDGES_COLS, rng, first_col=1,
                           forced=lambda r: [r, last] if r in (3, 13, 23, 29) else [r],
                           window=lambda r: (1, 300) if r in (19, 20, 21) else None)
    return indptr, indices, EDGES_COLS


def bulk():
    """2000 x 700 with Zipf-like degrees in 0 .. 70: bundles of many rows of equal and of unequal length, rows just above
    SPMM_SMAX, a tenth of the rows empty (the first and the last among them).  Returns (indptr, indices, n_cols)."""
    rng = np.random.default_rng(700)
    deg = np.minimum(rng.zipf(1.6, BULK_ROWS), BULK_MAX_DEGREE)
    deg[rng.random(BULK_ROWS) < 0.1] = 0
    deg[0] = deg[-1] = 0
    deg[1], deg[2] = BULK_MAX_DEGREE, 1
    indptr, indices = _csr(deg, BULK_COLS, rng)
    return indptr, indices, BULK_COLS


def boundary_matrix(n_cols):
    """200 rows of degree 1, 5, 40, 70, 130, 300 in turn, columns spread over [0, n_cols), every row holding the last column: the
    matrix of the 4 GiB table cases.  Returns (indptr, indices)."""
    rng = np.random.default_rng(n_cols)
    deg = np.array([(1, 5, 40, 70, 130, 300)[r % 6] for r in range(200)])
    return _csr(deg, n_cols, rng, forced=lambda r: [n_cols - 1])


# ---- the operands ---------------------------------------------------------------------------------------------------------
def data(mode, nnz, n_rows, n_cols, d, seed, n_add=N_ADD_MAX):
    """(vals [nnz], X [n_cols, d], addends n_add x [n_rows, d]) in float32.
    "int":  vals in {-2 .. 2} (stored zeros included), X and the addends integers of [-8, 8]: with a scale of INT_SCALES every
            partial sum of any order is an integer (times the scale) below 2^24 in magnitude -- exact in float32.
    "real": signed standard normals, every 97th stored value a zero."""
    rng = np.random.default_rng([seed, d, nnz])
    if mode == "int":
        vals = rng.integers(-INT_VAL_MAX, INT_VAL_MAX + 1, nnz)
        X = rng.integers(-INT_X_MAX, INT_X_MAX + 1, (n_cols, d))
        adds = [rng.integers(-INT_X_MAX, INT_X_MAX + 1, (n_rows, d)) for _ in range(n_add)]
    elif mode == "real":
        vals = rng.standard_normal(nnz)
        vals[::97] = 0.0  # a few stored zeros
        X = rng.standard_normal((n_cols, d))
        adds = [rng.standard_normal((n_rows, d)) for _ in range(n_add)]
    else:
        raise ValueError(mode)
    return vals.astype(np.float32), X.astype(np.float32), [a.astype(np.float32) for a in adds]


def int_scale(*key):
    """The scale of an "int" case: INT_SCALES in turn over the case's integer key."""
    return INT_SCALES[sum(int(k) for k in key) % len(INT_SCALES)]


# ---- the third generation's stream, walked as the kernel walks it ----------------------------------------------------------
def emulate(n_rows, X, d, packed):
    """spmm_stream_pack's output `packed` walked as csrc/spmm_bundle.hip:spmm_stream_kernel does: wave by wave, unit by unit,
    UN steps of G entries at a time; pieces go to their row or partial slot, bundles write one row per lane group, cut rows
    are added up from their slots.  Returns the float64 product [n_rows, d]; asserts that every row is written exactly once
    and that every wave with units owns the batches the kernel pre-loads."""
    G, UN, DW = packed["G"], packed["UN"], packed["DW"]
    cw = packed["cw"].reshape(-1, 2)
    cc, ww = cw[:, 0], cw[:, 1].copy().view(np.float32)
    ud = packed["ud"].reshape(-1, DW)
    wd = packed["wdesc"].reshape(-1, 4)
    Y = np.full((n_rows, d), np.nan)
    partial = np.full((max(packed["n_slots"], 1), d), np.nan)
    written = np.zeros(n_rows, int)
    n_batches = len(cw) // 64
    for w in range(len(wd)):
        sb, nb, u0, u1 = (int(v) for v in wd[w])
        pos = sb * 64
        # the kernel pre-loads batch 0 and batch min(1, nb - 1) of the run of every wave that has units: they must exist
        assert u1 <= u0 or (nb >= 1 and sb + nb <= n_batches), ("wave with units but no batch", w, sb, nb, u0, u1)
        for u in range(u0, u1):
            hdr = int(ud[u, 0])
            steps = (hdr & 0x7FFFFFFF) * UN
            e = slice(pos, pos + steps * G)
            terms = ww[e].astype(np.float64)[:, None] * np.asarray(X, dtype=np.float64)[cc[e]]
            acc = terms.reshape(steps, G, d).sum(0)  # lane group g takes entry step * G + g
            pos += steps * G
            assert pos <= (sb + nb) * 64, ("unit runs past its wave's batches", w, u)
            if hdr < 0:
                row, slot = int(ud[u, 1]), int(ud[u, 2])
                if slot >= 0:
                    partial[slot] = acc.sum(0)
                else:
                    Y[row] = acc.sum(0)
                    written[row] += 1
            else:
                for g in range(G):
                    a = int(ud[u, 1 + g])
                    if a < 0:
                        continue
                    r = a & 0x3FFFFFFF
                    Y[r] = 0.0 if a & 0x40000000 else acc[g]
                    written[r] += 1
    for i, r in enumerate(packed["crow"]):
        Y[r] = partial[packed["cptr"][i]:packed["cptr"][i + 1]].sum(0)
        written[r] += 1
    assert (written == 1).all(), written
    return Y
