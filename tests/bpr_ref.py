"""Host reference of the BPR loss and scatter kernels (gdmcf_bpr_loss_f32, gdmcf_bpr_grad_f32), written from their contract text
in include/gdmcf_hip.h -- numpy float64, no GPU, no gdmcf_amd import -- with the tables, the batches and the bounds that
tests/test_gpu_bpr_kernels.py runs the kernels on and tests/test_host_bpr_ref.py checks on the host.

  lane_group / WIDTHS      a row of d floats is served by LG = 2^ceil(log2(ceil(d / 4))) lanes (at most 64), G = 256 / LG lane
                           groups to a workgroup; the widths of every LG class, d > 256 takes more than one column pass
  Batch                    triples with their entries e = role * B + j, nodes, stable order and runs
  loss_ref / mode0_ref / mode1_ref     the header's formulas in float64
  dyadic_table / tails_table / real_table / int_table     the operands
  spread ... bad_ids       the batches, each built for a lane-group size
  x_bound / scatter_bound / mf_bound / reg_exact          how far float32 may be from the reference (derived below)
  check_loss / check_mode0 / check_mode1                  the comparisons of the GPU module, as functions, so that the host
                           module can show that they pass a float32 evaluation and fail the faults of loss32 / scatter32
"""
import math

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
F32, F64 = np.float32, np.float64
LGS = (1, 2, 4, 8, 16, 32, 64)
WIDTHS = {1: (1, 3, 4), 2: (5, 8), 4: (12, 16), 8: (20, 32), 16: (33, 64), 32: (100, 128), 64: (129, 256, 257, 260, 516)}
ALL_WIDTHS = tuple(d for lg in LGS for d in WIDTHS[lg])
SCATTER_WIDTHS = (4, 5, 16, 20, 33, 128, 129, 257, 260, 516)  # one per class, float4 and element-wise alternating, and all > 256
SMALL = (11, 7)  # n_users, n_items of the batches with long runs
WIDE = (300, 200)  # of `spread` and `bad_ids`
# Below x = -80, exp(x) < 2^-115 and coef = sigmoid(x) / B (B <= 2^11) leaves float32's normal range, where no relative error holds:
# such triples are held to 0 <= value <= value(-80) (1 + TRANS_CAP) instead (softplus and sigmoid increase with x).
DEEP_X = -80.0
TRANS_CAP = 16 * U  # no assertion on the device's expf / log1pf / division may be wider than this


def lane_group(d):
    chunks, lg = (d + 3) // 4, 1
    while lg < chunks and lg < 64:
        lg *= 2
    return lg


def column_passes(d):
    return -(-d // (4 * lane_group(d)))


# ---- batches --------------------------------------------------------------------------------------------------------------------
def order(users, pos, neg, n_users):
    """int32 [3B]: the entries e = role * B + j (role 0 user, 1 pos, 2 neg) sorted stably by users / pos + n_users / neg + n_users
    -- the sort key of gdmcf_amd.bpr._bpr_order, out-of-range ids included"""
    keys = np.concatenate([np.asarray(users, np.int64), np.asarray(pos, np.int64) + n_users, np.asarray(neg, np.int64) + n_users])
    return np.argsort(keys, kind="stable").astype(np.int32)


class Batch:
    def __init__(self, name, users, pos, neg, n_users, n_items):
        self.name, self.n_users, self.n_items = name, int(n_users), int(n_items)
        self.users, self.pos, self.neg = (np.ascontiguousarray(a, dtype=np.int64) for a in (users, pos, neg))
        assert self.users.ndim == 1 and self.users.shape == self.pos.shape == self.neg.shape and self.B > 0

    B = property(lambda self: self.users.shape[0])
    N = property(lambda self: self.n_users + self.n_items)

    def ok(self):
        """bool [B]: triples with all three ids in range"""
        return ((self.users >= 0) & (self.users < self.n_users) & (self.pos >= 0) & (self.pos < self.n_items) &
                (self.neg >= 0) & (self.neg < self.n_items))

    def nodes(self):
        """int64 [3B]: the node of every entry, -1 where the entry's own id is out of range"""
        u = np.where((self.users >= 0) & (self.users < self.n_users), self.users, -1)
        p = np.where((self.pos >= 0) & (self.pos < self.n_items), self.pos + self.n_users, -1)
        n = np.where((self.neg >= 0) & (self.neg < self.n_items), self.neg + self.n_users, -1)
        return np.concatenate([u, p, n])

    def order(self):
        return order(self.users, self.pos, self.neg, self.n_users)

    def runs(self):
        """[(node, start, length)]: maximal stretches of `order` whose entries share one valid node"""
        nd = self.nodes()[self.order()]
        out, k = [], 0
        while k < len(nd):
            e = k + 1
            while e < len(nd) and nd[e] == nd[k]:
                e += 1
            if nd[k] >= 0:
                out.append((int(nd[k]), k, e - k))
            k = e
        return out

    def multiplicity(self):
        """int64 [N]: entries per node (entries whose own id is out of range count nowhere)"""
        nd = self.nodes()
        return np.bincount(nd[nd >= 0], minlength=self.N)

    def clean(self):
        """the batch without its out-of-range triples"""
        ok = self.ok()
        return Batch(self.name + "_clean", self.users[ok], self.pos[ok], self.neg[ok], self.n_users, self.n_items)


def spread(B, seed=0):
    """random ids on 300 users and 200 items: runs of mostly one or two entries.  Users 0 .. 4 (the rows tails_table scales) are
    in it, from B = 18 on behind the triples that bad_ids spoils."""
    rng = np.random.default_rng(1000 + seed)
    U_, I_ = WIDE
    users = rng.integers(0, U_, B)
    first = 9 if B >= 18 else 0
    users[first:first + 5] = np.arange(5)[:B]
    return Batch("spread", users, rng.integers(0, I_, B), rng.integers(0, I_, B), U_, I_)


def hub_user(LG):
    """one user for all B = 2 LG + 3 triples: a run of B entries"""
    rng = np.random.default_rng(LG)
    B = 2 * LG + 3
    return Batch("hub_user", np.full(B, 5), rng.integers(0, SMALL[1], B), rng.integers(0, SMALL[1], B), *SMALL)


def hub_item(B):
    """pos = neg = item 3 for all triples: a run of 2 B entries, x = 0, coef = 0.5 / B, the mode-0 row of the item cancels"""
    rng = np.random.default_rng(B)
    return Batch("hub_item", rng.integers(0, SMALL[0], B), np.full(B, 3), np.full(B, 3), *SMALL)


MULTIPLE_RUNS = ("1", "LG-1", "LG", "LG+1", "2LG", "2LG+1")


def multiple_lengths(LG):
    return [n for n in (1, LG - 1, LG, LG + 1, 2 * LG, 2 * LG + 1) if n >= 1]


def multiples(LG):
    """users 0, 1, ... with runs of exactly 1, LG - 1 (LG > 1), LG, LG + 1, 2 LG and 2 LG + 1 entries; items at random"""
    rng = np.random.default_rng(LG)
    users = np.concatenate([np.full(n, u) for u, n in enumerate(multiple_lengths(LG))])
    rng.shuffle(users)
    B = len(users)
    return Batch("multiples", users, rng.integers(0, SMALL[1], B), rng.integers(0, SMALL[1], B), *SMALL)


def last_run_full(LG, k=1):
    """the highest node (the last item) has exactly k LG entries: the last k LG entries of `order`"""
    rng = np.random.default_rng(LG + k)
    n, last = k * LG, SMALL[1] - 1
    B = n + 2
    pos, neg = rng.integers(0, last, B), rng.integers(0, last, B)
    pos[: (n + 1) // 2] = last
    neg[1: 1 + n // 2] = last
    return Batch("last_run_full%d" % k, rng.integers(0, SMALL[0], B), pos, neg, *SMALL)


def straddle(LG):
    """user 10 has LG + 2 entries, the first of them at position G - 1 of `order` (the last lane group of workgroup 0): G - 1
    entries of users 0 .. 9 go before it"""
    rng = np.random.default_rng(LG)
    G = 256 // LG
    users = np.concatenate([np.arange(G - 1) % 10, np.full(LG + 2, 10)])
    rng.shuffle(users)
    B = len(users)
    return Batch("straddle", users, rng.integers(0, SMALL[1], B), rng.integers(0, SMALL[1], B), *SMALL)


def neighbours(LG):
    """the last user (LG entries: a whole chunk, so the walk's next chunk begins with another node's entries) and item 0 (keys
    n_users - 1 and n_users, adjacent) are both present and are distinct runs"""
    rng = np.random.default_rng(LG)
    B = LG + 4
    users = np.concatenate([np.full(LG, SMALL[0] - 1), rng.integers(0, SMALL[0] - 1, 4)])
    pos, neg = rng.integers(1, SMALL[1], B), rng.integers(1, SMALL[1], B)
    pos[0] = pos[B - 1] = neg[1] = 0
    return Batch("neighbours", users, pos, neg, *SMALL)


def bad_slots(n_users, n_items):
    """(triple slot, role, id): every role gets ids below and above its range, slot 3 has two of them.  pos / neg = -3 has the
    sort key of user n_users - 3 and user = n_users that of item 0: those entries sort next to a valid node's run."""
    return ((0, 0, -1), (1, 1, n_items), (2, 2, -3), (3, 0, n_users), (3, 2, 2 ** 40), (4, 1, -3), (5, 0, -3), (6, 2, n_items),
            (7, 1, 2 ** 40), (8, 0, n_users + 2))


def bad_ids(B, seed=0):
    """`spread` with out-of-range ids in its first triples -- all of bad_slots from B = 18 on, the first max(1, B // 2) slots'
    below that -- and, from B = 18 on, user n_users - 3 and item 0 (as pos and as neg) among the valid triples behind them"""
    b = spread(B, seed)
    users, pos, neg = b.users.copy(), b.pos.copy(), b.neg.copy()
    n_slots = 9 if B >= 18 else max(1, B // 2)
    for slot, role, value in bad_slots(*WIDE):
        if slot < n_slots:
            (users, pos, neg)[role][slot] = value
    if B >= 18:
        users[B - 1] = users[B - 4] = WIDE[0] - 3
        pos[B - 2] = neg[B - 3] = 0
    return Batch("bad_ids", users, pos, neg, *WIDE)


def scatter_batches(LG):
    """every batch of the scatter tests at lane-group size LG; 3 B is no multiple of G for `spread` and `bad_ids` (B = G + 1)"""
    G = 256 // LG
    return [spread(G + 1), hub_user(LG), hub_item(LG + 1), multiples(LG), last_run_full(LG, 1), last_run_full(LG, 2), straddle(LG),
            neighbours(LG), bad_ids(max(G + 1, 18))]


def loss_batches(LG):
    """spread, hub_item and bad_ids at B = 1, G + 1 and 128"""
    G = 256 // LG
    return [f(B) for B in (1, G + 1, 128) for f in (spread, hub_item, bad_ids)]


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def dyadic_table(N, d, seed):
    """[N, d] float32 with entries in {-2 .. 2} / 4, a column kept with probability min(1, 48 / d): products are multiples of
    1 / 16 of at most 1 / 4, so every dot product, squared norm and difference of them is exact in float32 in any order.  The
    last float4 chunk and column 256 are always kept: a dropped last chunk or second column pass changes the result."""
    rng = np.random.default_rng([seed, d])
    T = rng.integers(-2, 3, (N, d)).astype(F64) / 4
    keep = rng.random(d) < min(1.0, 48.0 / d)
    keep[4 * ((d - 1) // 4):] = True
    keep[256:257] = True
    return (T * keep).astype(F32)


def tails_table(N, d, seed):
    """dyadic_table with user rows 0 .. 4 times 32: |x| beyond 20 on both sides, still exact"""
    T = dyadic_table(N, d, seed)
    T[:5] *= 32
    return T


def real_table(N, d, seed):
    return np.random.default_rng([seed, d, 7]).standard_normal((N, d)).astype(F32)


def int_table(N, d, seed, lo=-3, hi=3):
    return np.random.default_rng([seed, d, 11]).integers(lo, hi + 1, (N, d)).astype(F32)


def dyadic_coef(B, seed):
    """k / 64 with k in -8 .. 8, zeros included: with a dyadic table every mode-0 row is exact"""
    return (np.random.default_rng([seed, B]).integers(-8, 9, B) / 64).astype(F32)


# ---- references -----------------------------------------------------------------------------------------------------------------
def _rows(b):
    ok = b.ok()
    return ok, np.where(ok, b.users, 0), b.n_users + np.where(ok, b.pos, 0), b.n_users + np.where(ok, b.neg, 0)


def loss_ref(M, E0, b):
    """dict: ok [B]; x, soft, coef, rg [B] float64 (0 for a triple with an id out of range); mf, reg; flag; xmag [B] =
    sum |a| |b| + sum |a| |c|, the magnitude x_bound needs"""
    T, E = np.asarray(M, F64), np.asarray(E0, F64)
    ok, u, p, n = _rows(b)
    x = (T[u] * T[n]).sum(1) - (T[u] * T[p]).sum(1)
    z = np.exp(np.minimum(x, 20.0))
    soft = np.where(x > 20.0, x, np.log1p(z))  # torch.nn.functional.softplus: beta 1, threshold 20
    sig = np.where(x > 20.0, 1.0, z / (1.0 + z))  # ... and its derivative
    rg = (E[u] ** 2).sum(1) + (E[p] ** 2).sum(1) + (E[n] ** 2).sum(1)
    x, soft, sig, rg = (np.where(ok, v, 0.0) for v in (x, soft, sig, rg))
    xmag = (np.abs(T[u]) * np.abs(T[p])).sum(1) + (np.abs(T[u]) * np.abs(T[n])).sum(1)
    return dict(ok=ok, x=x, soft=soft, coef=sig / b.B, rg=rg, mf=soft.sum() / b.B, reg=0.5 * rg.sum() / b.B,
                flag=int(not ok.all()), xmag=xmag)


def mode0_ref(b, coef, src, out0):
    """(out float64 [N, d], written bool [N], mag [N, d], count [N]): out[node] = the header's sum over the node's entries, rows
    of no entry as in out0; mag = sum_i |w_i| (|a_i| + |b_i|), count = entries per node.  A triple with an id out of range
    contributes 0 (its coef is 0); an entry whose own id is out of range writes nothing."""
    S = np.asarray(src, F64)
    ok, u, p, n = _rows(b)
    c = np.where(ok, np.asarray(coef, F64), 0.0)[:, None]
    nd, B = b.nodes(), b.B
    acc, mag = np.zeros((b.N, S.shape[1])), np.zeros((b.N, S.shape[1]))
    terms = ((c * (S[n] - S[p]), np.abs(c) * (np.abs(S[n]) + np.abs(S[p]))), (-c * S[u], np.abs(c * S[u])),
             (c * S[u], np.abs(c * S[u])))
    for role, (term, size) in enumerate(terms):
        node = nd[role * B:(role + 1) * B]
        np.add.at(acc, node[node >= 0], term[node >= 0])
        np.add.at(mag, node[node >= 0], size[node >= 0])
    count = b.multiplicity()
    out = np.array(out0, F64)
    out[count > 0] = acc[count > 0]
    return out, count > 0, mag, count


def mode1_ref(b, src, out0, scale, zero0=None):
    """(out, zero): out[node] += scale * multiplicity * src[node]; zero_rows[node] cleared for exactly the batch's nodes"""
    count = b.multiplicity()
    out = np.array(out0, F64) + scale * count[:, None] * np.asarray(src, F64)
    zero = None
    if zero0 is not None:
        zero = np.array(zero0, F64)
        zero[count > 0] = 0.0
    return out, zero


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def x_bound(ref, d):
    """|x32 - x| <= 2 (d + 2) u (sum |a| |b| + sum |a| |c|): each dot product is d products and d - 1 additions in some order,
    every rounding at most u of a partial sum below sum |a| |b|; (1 + u)^(d + 1) - 1 < 2 (d + 1) u for the sizes here, and the
    final subtraction adds one more u of the two sums (tests/test_gpu_bpr_negs.py derives the same form for one score)"""
    return 2 * (d + 2) * U * ref["xmag"]


def scatter_bound(mag, count):
    """per element 2 (n_run + 3) u sum_i |w_i| (|a_i| + |b_i|): a term is a subtraction, a product and an addition into the
    accumulator (3 roundings, or fewer when the compiler contracts), then at most n_run - 1 further additions touch it"""
    return 2 * (count[:, None] + 3) * U * mag


def mf_bound(ws, B):
    """|mf - mean64(ws[:B])| <= (ceil(B / 256) + 9) u sum |ws_j| / B: the serial additions of one thread, eight tree levels, the
    division"""
    return (math.ceil(B / 256) + 9) * U * np.abs(np.asarray(ws[:B], F64)).sum() / B


def reg_exact(rg64, B):
    """the kernel's 0.5f * s / (float) B with s the exact sum (dyadic tables: s is a float32 number)"""
    s = F32(np.asarray(rg64, F64).sum())
    assert float(s) == float(np.asarray(rg64, F64).sum())
    return F32(F32(0.5) * s) / F32(B)


# ---- the comparisons of the GPU module ------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def check_loss(coef, ws, mf, reg, ref, d, tol, exact_x=True, exact_reg=True):
    """coef, ws = (soft, rg), mf, reg of one call against loss_ref's dict.  exact_x: the tables make x exact, the only error is
    the device's expf, log1pf and division, relative `tol` (one number, or one for coef and one for soft); otherwise x_bound
    is carried through |sigmoid'| <= 1 / 4 and |softplus'| <= 1 on top of it.  Returns the observed (max |coef / ref - 1|, max |soft / ref - 1|) over the triples above
    DEEP_X, what the tolerance is measured from."""
    tol_c, tol_s = tol if isinstance(tol, tuple) else (tol, tol)
    assert 0 < tol_c <= TRANS_CAP and 0 < tol_s <= TRANS_CAP
    coef, ws = np.asarray(coef, F64), np.asarray(ws, F64)
    B = coef.shape[0]
    soft, rg, ok = ws[:B], ws[B:], ref["ok"]
    assert ws.shape == (2 * B,) and np.isfinite(coef).all() and np.isfinite(ws).all()
    assert (coef[~ok] == 0).all() and (soft[~ok] == 0).all() and (rg[~ok] == 0).all(), "an out-of-range triple contributes"
    xb = np.zeros(B) if exact_x else x_bound(ref, d)
    shallow = ok & (ref["x"] - xb >= DEEP_X)
    deep = ok & ~shallow
    cb, sb = tol_c * ref["coef"] + xb / (4 * B), tol_s * ref["soft"] + xb
    ce, se = np.abs(coef - ref["coef"]), np.abs(soft - ref["soft"])
    assert (ce[shallow] <= cb[shallow]).all(), ("coef", (ce[shallow] / ref["coef"][shallow]).max() / U)
    assert (se[shallow] <= sb[shallow]).all(), ("soft", (se[shallow] / ref["soft"][shallow]).max() / U)
    cap = math.exp(DEEP_X) * (1 + TRANS_CAP)
    assert (coef[deep] >= 0).all() and (coef[deep] <= cap / B).all() and (soft[deep] >= 0).all() and (soft[deep] <= cap).all()
    if exact_reg:
        assert same_bits(ws[B:], ref["rg"]), "rg"
        assert same_bits(reg, reg_exact(ref["rg"], B)), ("reg", float(reg), ref["reg"])
    else:  # 3 d squares and their sum, all positive: relative 2 (3 d + 2) u per triple; then the reduction of mf_bound
        assert (np.abs(rg - ref["rg"]) <= 2 * (3 * d + 2) * U * ref["rg"]).all(), "rg"
        assert abs(float(reg) - ref["reg"]) <= (2 * (3 * d + 2) + math.ceil(B / 256) + 10) * U * ref["reg"], "reg"
    own = mf_bound(ws, B)
    assert abs(float(mf) - soft.sum() / B) <= own, ("mf of ws", float(mf), soft.sum() / B, own)
    assert abs(float(mf) - ref["mf"]) <= own + (sb[shallow].sum() + cap * deep.sum()) / B, ("mf", float(mf), ref["mf"])
    if not shallow.any():
        return 0.0, 0.0
    return float((ce[shallow] / ref["coef"][shallow]).max()), float((se[shallow] / ref["soft"][shallow]).max())


def check_mode0(got, b, coef, src, out0, exact=True):
    """got [N, d] after a mode-0 call on out0: rows of no entry keep out0's bits; the others equal the float64 sum bit for bit
    (exact operands) or lie inside scatter_bound"""
    want, written, mag, count = mode0_ref(b, coef, src, out0)
    assert same_bits(np.asarray(got)[~written], np.asarray(out0)[~written]), "a row of no entry was written"
    if exact:
        assert same_bits(np.asarray(got)[written], want[written].astype(F32)), "mode 0 rows"
    else:
        err = np.abs(np.asarray(got, F64) - want)[written]
        assert (err <= scatter_bound(mag, count)[written]).all(), "mode 0 rows beyond the scatter bound"


def check_mode1(got, got_zero, b, src, out0, scale, zero0=None):
    want, zero = mode1_ref(b, src, out0, scale, zero0)
    assert same_bits(got, want.astype(F32)), "mode 1 rows"
    if zero0 is not None:
        assert same_bits(got_zero, zero.astype(F32)), "zero_rows"


# ---- float32 evaluations in index order, with the faults the comparisons must reject --------------------------------------------
FAULTS = ("drop", "dup", "cut", "neighbour", "chunk")


def dot32(a, b, cols=None):
    """row-wise float32 dot product, columns added one after the other"""
    s = np.zeros(a.shape[0], F32)
    for c in range(a.shape[1] if cols is None else cols):
        s = (s + a[:, c] * b[:, c]).astype(F32)
    return s


def loss32(M, E0, b, fault=None, scramble=None):
    """(coef, ws, mf, reg) float32: dot products column by column (or in the column order `scramble`), softplus / sigmoid
    correctly rounded from the float32 x, the sums of mf and reg one term after the other.  fault "chunk": the last float4
    column chunk is left out of every dot product."""
    M, E0 = np.asarray(M, F32), np.asarray(E0, F32)
    if scramble is not None:
        M, E0 = M[:, scramble], E0[:, scramble]
    d = M.shape[1]
    cols = 4 * ((d - 1) // 4) if fault == "chunk" else d
    ok, u, p, n = _rows(b)
    x = (dot32(M[u], M[n], cols) - dot32(M[u], M[p], cols)).astype(F64)
    z = np.exp(np.minimum(x, 20.0))
    soft = np.where(ok, np.where(x > 20.0, x, np.log1p(z)), 0).astype(F32)
    coef = (np.where(ok, np.where(x > 20.0, 1.0, z / (1.0 + z)), 0).astype(F32) / F32(b.B)).astype(F32)
    rg = np.where(ok, (dot32(E0[u], E0[u], cols) + dot32(E0[p], E0[p], cols)).astype(F32) + dot32(E0[n], E0[n], cols), 0).astype(F32)
    s0 = s1 = F32(0)
    for j in range(b.B):
        s0, s1 = F32(s0 + soft[j]), F32(s1 + rg[j])
    return coef, np.concatenate([soft, rg]), F32(s0 / F32(b.B)), F32(F32(F32(0.5) * s1) / F32(b.B))


def scatter32(b, mode, coef, src, out0, LG, scale=0.0, zero0=None, fault=None):
    """(out, zero) float32: every run of `order` walked entry by entry in sorted order.  Faults, each applied to every run it can
    apply to: "drop" leaves out a run's last entry (runs of two or more), "dup" takes it twice, "cut" stops after LG entries,
    "neighbour" gives the row the entries of the run behind it, "chunk" leaves the last float4 column chunk unwritten."""
    src, out = np.asarray(src, F32), np.array(out0, F32)
    zero = None if zero0 is None else np.array(zero0, F32)
    d, B, od, runs = src.shape[1], b.B, b.order(), b.runs()
    cols = slice(0, 4 * ((d - 1) // 4) if fault == "chunk" else d)
    ok, u, p, n = _rows(b)
    for r, (node, start, length) in enumerate(runs):
        if fault == "neighbour" and r + 1 < len(runs):
            start, length = runs[r + 1][1:]
        ents = [int(e) for e in od[start:start + length]]
        if fault == "drop" and len(ents) >= 2:
            ents = ents[:-1]
        if fault == "dup":
            ents = ents + ents[-1:]
        if fault == "cut":
            ents = ents[:LG]
        if mode == 1:
            s = F32(F32(scale) * F32(len(ents)))
            out[node, cols] = (out[node, cols] + s * src[node, cols]).astype(F32)
            if zero is not None:
                zero[node, cols] = 0
            continue
        acc = np.zeros(d, F32)
        for e in ents:
            role, j = divmod(e, B)
            c = F32(coef[j]) if ok[j] else F32(0)
            if role == 0:
                acc = (acc + c * (src[n[j]] - src[p[j]]).astype(F32)).astype(F32)
            else:
                acc = (acc + (-c if role == 1 else c) * src[u[j]]).astype(F32)
        out[node, cols] = acc[cols]
    return out, zero
