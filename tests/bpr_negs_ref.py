"""Host model of gdmcf_bpr_sample_pool_f32's draws (several negatives per positive, each the best of a pool), restated from the
contract text in include/gdmcf_hip.h on top of tests/draws_ref.py -- numpy only, no GPU, no gdmcf_amd import -- and the small
graphs the sampler's tests share.  Used by tests/test_gpu_bpr_negs.py and tests/test_host_bpr_negs.py.

Layout: triple j owns the Philox blocks with counters (j, 0, 7, offset), (j, 1, 7, offset), ...  Word x of block 0 draws the
positive.  Candidate number q = k * pool + c (negative slot k, pool position c) takes word y, z, w of block 0 for q = 0, 1, 2
and word (q - 3) % 4 of block 1 + (q - 3) // 4 for q >= 3.
"""
import numpy as np

from tests import draws_ref as D


def candidate_place(q):
    """(block, word) of candidate number q"""
    return (0, q + 1) if q < 3 else (1 + (q - 3) // 4, (q - 3) % 4)


def pool_triples(indptr, indices, users, n_users, n_items, seed, offset, n_negs, pool, M=None):
    """(pos [B], neg [B, n_negs], flag, cands [B, n_negs, pool]).  cands: every candidate in the order drawn.  With pool > 1 the
    slot keeps its first candidate unless a later one scores strictly greater; scores are <M[u], M[n_users + i]> in float64 (exact
    for the integer-valued tables the exact tests use).  -1 everywhere and a raised flag for a user outside [0, n_users) or with
    deg <= 0 or deg >= n_items."""
    users = np.asarray(users, dtype=np.int64)
    B = users.shape[0]
    n_blocks = 1 + candidate_place(n_negs * pool - 1)[0]
    words = np.stack(D.block(np.arange(B, dtype=np.uint64)[:, None], np.arange(n_blocks, dtype=np.uint64)[None, :], D.STREAM_BPR,
                             offset, seed), axis=-1)  # [B, n_blocks, 4]
    pos = np.full(B, -1, dtype=np.int64)
    neg = np.full((B, n_negs), -1, dtype=np.int64)
    cands = np.full((B, n_negs, pool), -1, dtype=np.int64)
    flag = 0
    T = None if M is None else np.asarray(M, dtype=np.float64)
    for j, u in enumerate(users.tolist()):
        deg = int(indptr[u + 1] - indptr[u]) if 0 <= u < n_users else 0
        if deg <= 0 or deg >= n_items:
            flag = 1
            continue
        row = np.asarray(indices[int(indptr[u]):int(indptr[u]) + deg])
        pos[j] = int(row[D.mulhi(words[j, 0, 0], deg)])
        for k in range(n_negs):
            for c in range(pool):
                blk, word = candidate_place(k * pool + c)
                cands[j, k, c] = D.bpr_negative(row, D.mulhi(words[j, blk, word], n_items - deg))
            best = int(cands[j, k, 0])
            if pool > 1:
                best_score = float(T[u] @ T[n_users + best])
                for c in range(1, pool):
                    s = float(T[u] @ T[n_users + int(cands[j, k, c])])
                    if s > best_score:  # (False for a NaN)
                        best, best_score = int(cands[j, k, c]), s
            neg[j, k] = best
    return pos, neg, flag, cands


def edge_graph():
    """37 users x 53 items: rows of 1-6 items, user 3 with 52 items (every negative is item 17, its one free item), user 5 with
    one item, user 7 with none and user 11 with all 53 (those two cannot be drawn for: -1 and the flag).  (indptr int64, indices
    int32, n_users, n_items, users): 33 user ids with repeats, the two ineligible users and one id out of range among them."""
    rng = np.random.default_rng(7)
    U, It = 37, 53
    rows = [np.sort(rng.choice(It, size=int(rng.integers(1, 7)), replace=False)) for _ in range(U)]
    rows[3] = np.array([i for i in range(It) if i != 17])
    rows[5] = np.array([40])
    rows[7] = np.zeros(0, np.int64)
    rows[11] = np.arange(It)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    users = np.concatenate([[3, 3, 5, 5, 7, 11, U, 0, 0, 0, 36, 36], rng.integers(0, U, 21)]).astype(np.int64)
    assert users.shape == (33,)
    return indptr, indices, U, It, users


# the 5 x 12 graph of tests/test_gpu_bpr.py::test_sampler_properties: degrees 1, 3, 6, 11 and 0
PROPERTY_ROWS = [[4], [0, 5, 11], [1, 2, 3, 7, 8, 10], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11], []]
PROPERTY_ITEMS = 12


def property_graph():
    """(indptr int64, indices int32, n_users, n_items, users): 2 000 drawn users, 500 of each of the four eligible ones, sorted"""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in PROPERTY_ROWS])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, np.int32) for r in PROPERTY_ROWS]).astype(np.int32)
    return indptr, indices, len(PROPERTY_ROWS), PROPERTY_ITEMS, np.repeat(np.arange(4, dtype=np.int64), 500)


def check_uniform_negatives(users, neg):
    """Every negative outside its user's row and inside [0, n_items); per user the count of each free item within 5 binomial
    standard deviations of uniform (about 27 cells, a two-sided 5 sigma tail of 6e-7 each: a correct sampler fails this for one
    seed in about 60 000)."""
    for u in range(4):
        drawn = neg[users == u].reshape(-1)
        free = [i for i in range(PROPERTY_ITEMS) if i not in PROPERTY_ROWS[u]]
        assert np.isin(drawn, free).all(), u
        n, p = drawn.size, 1.0 / len(free)
        sigma = np.sqrt(n * p * (1 - p))
        for i in free:
            k = int((drawn == i).sum())
            assert k > 0 and abs(k - n * p) <= 5 * sigma, (u, i, k, n * p, sigma)


def check_best_of_three(users, neg, cands):
    """Scores that grow with the item id and pool = 3: the chosen negative is the largest of its pool, and the m-th smallest of a
    user's F free items is chosen with probability ((m + 1)^3 - m^3) / F^3 -- counts within 5 binomial standard deviations."""
    assert (neg == cands.max(-1)).all()
    for u in range(4):
        drawn = neg[users == u].reshape(-1)
        free = [i for i in range(PROPERTY_ITEMS) if i not in PROPERTY_ROWS[u]]
        assert np.isin(drawn, free).all(), u
        n, F = drawn.size, len(free)
        for m, i in enumerate(free):
            p = ((m + 1) ** 3 - m ** 3) / F ** 3
            k = int((drawn == i).sum())
            assert abs(k - n * p) <= 5 * np.sqrt(n * p * (1 - p)), (u, i, k, n * p)


def increasing_score_table(n_users, n_items, d):
    """M[u] = e_0, M[n_users + i] = i e_0: the score of item i is i"""
    M = np.zeros((n_users + n_items, d), np.float32)
    M[:n_users, 0] = 1.0
    M[n_users:, 0] = np.arange(n_items)
    return M
