"""CPU (-m "not gpu"): the host model of the in-kernel draws (tests/draws_ref.py) against published Philox4x32-10 vectors and
against its own definitions, and the C entries' refusal of Philox offsets that do not fit the counter (56 bits)."""
import numpy as np
import pytest

from gdmcf_amd import _lib
from tests import draws_ref as R

# Random123 known-answer vectors (kat_vectors, philox4x32 10 rounds): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, out in KAT:
        assert tuple(int(w) for w in R.philox4x32_10(ctr, key)) == out
    # vectorised over arrays: the three vectors at once, and broadcasting of a scalar key
    got = R.philox4x32_10([np.array([k[0][i] for k in KAT]) for i in range(4)], [np.array([k[1][i] for k in KAT]) for i in range(2)])
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KAT]
    got = R.philox4x32_10((np.zeros((2, 3)), 0, 0, 0), (0, 0))
    assert got[0].shape == (2, 3) and got[0].dtype == np.uint32 and int(got[3][1, 2]) == KAT[0][2][3]


def test_counter_keeps_the_high_offset_bits_above_the_stream_id():
    assert R.counter(7, 2, 3, 5) == (7, 2, 3, 5)                       # offsets below 2^32: the counters they always had
    assert R.counter(7, 2, 3, (1 << 32) - 1) == (7, 2, 3, 0xFFFFFFFF)
    assert R.counter(7, 2, 3, (1 << 40) + 5) == (7, 2, 3 | (0x100 << 8), 5)
    assert R.counter(0, 0, 255, (1 << 56) - 1) == (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)
    with pytest.raises(ValueError):
        R.counter(0, 0, 0, 1 << 56)
    with pytest.raises(ValueError):
        R.counter(0, 0, 256, 0)
    # the block is the Philox block of that counter under the key (seed low, seed high)
    seed = 0xa4093822 | (0x299f31d0 << 32)
    got = R.block(0x243f6a88, 0x85a308d3, 0x2e, 0x03707344 | (0x13198a << 32), seed)
    assert tuple(int(w) for w in got) == KAT[2][2]
    lo, hi = R.block(1, 2, 0, 5, 9), R.block(1, 2, 0, (1 << 40) + 5, 9)
    assert tuple(map(int, lo)) != tuple(map(int, hi))


def test_normals_layout_and_edges():
    B, I, seed, off = 3, 11, 1234, 77
    z = R.normals(B, I, 4, seed, off)
    assert z.shape == (B, I) and z.dtype == np.float64
    # element (b, i): normal i & 3 of block (i >> 2, b): pairs (x, y) -> cos, sin and (z, w) -> cos, sin
    x, y, zz, w = (int(v) for v in R.block(2, 1, 4, off, seed))

    def bm(a, b):
        u1 = float(np.float32(np.float32(a) + np.float32(1)) * np.float32(2.0 ** -32))
        u2 = float(np.float32(b) * np.float32(2.0 ** -32))
        r = np.sqrt(-2.0 * np.log(u1))
        return r * np.cos(2 * np.pi * u2), r * np.sin(2 * np.pi * u2)
    assert np.allclose(z[1, 8:11], [*bm(x, y), bm(zz, w)[0]], rtol=0, atol=1e-15)
    # the word 0xFFFFFFFF gives u1 = 1 and a normal of exactly 0; the word 0 gives the largest radius, sqrt(64 ln 2)
    n0, n1 = R.box_muller(np.array([0xFFFFFFFF, 0], dtype=np.uint32), np.array([0x40000000, 0], dtype=np.uint32))
    assert n0[0] == 0.0 and n1[0] == 0.0
    assert n0[1] == np.sqrt(64 * np.log(2.0)) and n1[1] == 0.0
    # a million draws: mean and variance of N(0,1) (4 sigma of the estimators)
    big = R.normals(4, 250000, 0, 5, 1)
    assert abs(big.mean()) < 4e-3 and abs(big.var() - 1.0) < 4 * np.sqrt(2e-6)


def test_keep_mask_definitions():
    B, I, seed, off = 2, 2500, 99, 3
    assert R.keep_mask(B, I, 0.0, seed, off).all()          # threshold 65536: every 16-bit uniform is below it
    assert R.keep_threshold(0.0) == 65536
    assert R.keep_threshold(0.5) == 32768                    # exact
    assert R.keep_threshold(0.3) == 45875                    # round(0.7 * 65536 = 45875.2)
    k = R.keep_mask(B, I, 0.5, seed, off)
    # element (b, i) from the definition, one at a time: half (i >> 10) & 1 of word i & 3 of block ((i & ~1024) >> 2, b, 1, offset)
    for b, i in [(0, 0), (1, 3), (0, 1023), (1, 1024), (0, 1027), (1, 2047), (0, 2048), (1, 2499)]:
        word = int(R.block((i & ~1024) >> 2, b, 1, off, seed)[i & 3])
        half = (word >> 16) if (i >> 10) & 1 else (word & 0xFFFF)
        assert bool(k[b, i]) == (half < 32768), (b, i)
    # columns i and i + 1024 share a block: the low and the high half of the same word
    i = 5
    word = int(R.block(i >> 2, 1, 1, off, seed)[i & 3])
    assert bool(k[1, i]) == ((word & 0xFFFF) < 32768) and bool(k[1, i + 1024]) == ((word >> 16) < 32768)
    assert abs(R.keep_mask(8, 50000, 0.3, seed, off).mean() - 45875 / 65536) < 4 * np.sqrt(0.21 / 400000)


def test_class_draws_definitions():
    B, I = 4, 9
    c = (np.arange(B * I).reshape(B, I) % 3 == 0).astype(np.uint8)
    ts = np.array([0, B, 1, 3])
    # a = 1 (t = B): P(1) = [c == 1] exactly, the draw reproduces the class; a = 0: P(1) = 1 - e for both classes
    s = R.class_draws(c, ts, B, 0.3, 3, 11, 2)
    assert (s[1] == c[1]).all()
    p1 = R.class_p1(c, ts, B, 0.3)
    assert p1.dtype == np.float32 and (p1[0] == np.float32(1.0 - float(np.float32(0.3)))).all()
    assert (R.class_draws(c, ts, B, 0.0, 3, 11, 2)[0] == 1).all()     # e = 0, a = 0: class 1 with probability 1
    assert (R.class_draws(c, ts, B, 1.0, 3, 11, 2)[0] == 0).all()     # e = 1, a = 0: class 0
    w = int(R.block(1, 2, 3, 2, 11)[2])                                # element (2, 6)
    assert int(s[2, 6]) == int(np.float32(w >> 8) * np.float32(2.0 ** -24) < p1[2, 6])


def test_timestep_search_edges():
    T = 7
    p = np.array([0.05, 0.3, 0.05, 0.2, 0.1, 0.25, 0.05])
    below_one = 1.0 - 2.0 ** -53
    assert R.timesteps_from_uniforms([0.0, below_one], T).tolist() == [0, T - 1]
    assert R.timesteps_from_uniforms([0.0, below_one], T, p).tolist() == [0, T - 1]
    assert R.timesteps_from_uniforms([0.0, below_one], 1).tolist() == [0, 0]
    cdf = np.cumsum(p)
    # just below / at a cdf step: the first index whose cdf EXCEEDS the point
    u = np.array([np.nextafter(cdf[1], 0.0), cdf[1]]) / cdf[-1]
    pts = u * cdf[-1]
    assert R.timesteps_from_uniforms(u, T, p).tolist() == [int(np.argmax(cdf > x)) for x in pts]
    u = R.timestep_uniforms(1000, 3, 4)
    assert u.min() >= 0.0 and u.max() < 1.0
    x, y, _, _ = (int(v) for v in R.block(17, 0, 2, 4, 3))
    assert u[17] == (x * 2.0 ** 32 + y) * 2.0 ** -64
    t = R.timesteps(1000, T, 3, 4, p)
    assert np.abs(np.bincount(t, minlength=T) / 1000.0 - p).max() < 4 * np.sqrt(0.25 / 1000)


def test_bpr_negative_covers_exactly_the_absent_items():
    n_items = 9
    row = np.array([1, 2, 5, 8], dtype=np.int32)
    absent = [i for i in range(n_items) if i not in row.tolist()]
    assert [R.bpr_negative(row, r) for r in range(n_items - len(row))] == absent
    indptr = np.array([0, 4, 4, 4 + n_items], dtype=np.int64)            # degrees 4, 0, n_items
    indices = np.concatenate([row, np.arange(n_items, dtype=np.int32)])
    users = np.zeros(400, dtype=np.int64)
    pos, neg, flag = R.bpr_triples(indptr, indices, users, 3, n_items, 5, 1)
    assert flag == 0 and set(pos.tolist()) == set(row.tolist()) and set(neg.tolist()) == set(absent)
    x, y, _, _ = (int(v) for v in R.block(3, 0, 7, 1, 5))
    assert pos[3] == row[(x * 4) >> 32] and neg[3] == absent[(y * 5) >> 32]
    pos, neg, flag = R.bpr_triples(indptr, indices, np.array([0, 1, 2, 3, -1]), 3, n_items, 5, 1)
    assert flag == 1 and pos[0] >= 0 and neg[0] >= 0
    assert pos[1:].tolist() == [-1] * 4 and neg[1:].tolist() == [-1] * 4


def test_entries_refuse_offsets_beyond_56_bits():
    """Every entry that takes a Philox offset returns GDMCF_E_SHAPE for offset >= 2^56, before it looks at a pointer; 2^56 - 1
    passes that check (the null pointers are refused next, or the call succeeds where it only fills a host block)."""
    lib = _lib.load()
    big, ok = 1 << 56, (1 << 56) - 1

    def entries(o, o2=None):
        o2 = o if o2 is None else o2
        return {
            "prep_input": lib.gdmcf_dnn_prep_input_f32(None, 8, None, None, None, 9, None, 0, 0, None, 0, 0.5, 1, o, 0, None, None,
                                                       0, 2, 8, None, 8, None, 0, None, None, None),
            "prep_input_csr": lib.gdmcf_dnn_prep_input_csr_f32(None, None, None, None, None, None, 0, None, 0, 0, None, 0, 0.5, 1,
                                                               o, None, None, 0, 2, 8, None, 8, None, None, 0, None),
            "onehot_prep_input_csr/noise": lib.gdmcf_onehot_prep_input_csr_f32(
                None, None, None, None, 0.3, None, 0, 1, o, None, 0, None, 0, None, 0, 0.5, 0, None, None, 0, 2, 8, None, 16, None,
                None, 0, None),
            "onehot_prep_input_csr/prep": lib.gdmcf_onehot_prep_input_csr_f32(
                None, None, None, None, 0.3, None, 0, 1, 0, None, 0, None, 0, None, 0, 0.5, o, None, None, 0, 2, 8, None, 16, None,
                None, 0, None),
            "onehot_noise": lib.gdmcf_onehot_noise_f32(None, 8, None, 2, 8, 0.3, None, 0, 1, o, None, 16, None, 0, None),
            "randn": lib.gdmcf_randn_f32(None, 8, 2, 8, 0, 1, o, None),
            "graph_guided_step": lib.gdmcf_graph_guided_step_u8(None, 8, None, 2, 8, 0.3, None, 0, None, None, 0, 1, o, None, 0,
                                                                None, None),
            "bpr_sample": lib.gdmcf_bpr_sample_f32(None, None, None, 4, 3, 5, 1, o, None, None, None, None),
            "cat_prep_input": lib.gdmcf_cat_prep_input_f32(None, 8, None, 16, None, None, None, 0, None, 0, 0, None, 0, 0.5, 1, o,
                                                           None, None, None, None, 10, 2, 8, None, 20, None, 8, None, None),
            "cat_prep_input_csr/noise": lib.gdmcf_cat_prep_input_csr_f32(
                None, None, None, None, 0.3, None, 0, o, None, None, None, 0, None, 0, 0, None, 0, 0.5, 1, 0, None, None, None,
                None, 10, 2, 8, None, 20, None, 8, None, None, 1, None, 1, None),
            "cat_prep_input_csr/prep": lib.gdmcf_cat_prep_input_csr_f32(
                None, None, None, None, 0.3, None, 0, 0, None, None, None, 0, None, 0, 0, None, 0, 0.5, 1, o, None, None, None,
                None, 10, 2, 8, None, 20, None, 8, None, None, 1, None, 1, None),
            "cat_grad": lib.gdmcf_cat_grad_f32(None, 8, None, 8, None, 16, 0, None, 0, 0.5, 1, o, 2, 8, None, 0, None, None, None),
            "cat_grad_bits": lib.gdmcf_cat_grad_bits_f32(None, 8, None, 8, None, 1, None, 1, 0, None, 0, 0.5, 1, o, 2, 8, None, 0,
                                                         None, None, None),
        }

    refused = entries(big)
    assert all(rc == _lib.E_SHAPE for rc in refused.values()), refused
    assert "2^56" in lib.gdmcf_last_error().decode()
    passed = entries(ok)
    assert all(rc == _lib.E_ARG for rc in passed.values()), passed
    # the sampler has no pointer check behind its shape checks: only the refusal is exercised here
    assert lib.gdmcf_sample_timesteps(None, None, 4, 2, 3, 0.001, 1, big, None, None, None, None) == _lib.E_SHAPE
    # the graph step state's two offsets
    assert lib.gdmcf_graph_state_init(None, big, 0, 0, 0, 0, None) == _lib.E_SHAPE
    assert lib.gdmcf_graph_state_init(None, 0, big, 0, 0, 0, None) == _lib.E_SHAPE
    assert lib.gdmcf_graph_state_init(None, ok, ok, 0, 0, 0, None) == _lib.E_ARG
