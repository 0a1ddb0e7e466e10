"""CPU (-m "not gpu"): the host models of tests/dr_ref.py, which tests/test_gpu_dr_edges.py holds the register-streaming weight-
gradient kernels to.

  * dr_tn_plan equals the library's own plan (gdmcf_debug_dr_tn_plan: dr_tn_prepare on a scratch product) for every batch row
    count 128 .. 1100, and the case table is what both say;
  * the twelve cases cover every ring depth with the AdamW update in the k loop (stream) and at the end of the tile (spot), both
    sides of the nine-round boundary for D = 8 and D = 9, padded k-steps and a batch tail (B % 4 != 0) in both modes;
  * the product bound passes a float32 evaluation in the kernels' k order on the case operands, and fails one dropped term, one
    duplicated term and a row taken from its neighbour.
"""
import ctypes

import numpy as np
import pytest

from gdmcf_amd import _lib
from tests import dr_ref as D

N_SWEEP, K_SWEEP = 1024, 2048  # the GPU module's sweep shape: 16 x 32 tiles, the fewest the kernels take


def lib_plan(B, N=N_SWEEP, K=K_SWEEP, lddz=None, lda=None, ldw=None, bias_col=0, fused=0):
    """(taken, depth, ksp, tiles_m, tiles_n, m_fastest, has_bias) of gdmcf_debug_dr_tn_plan"""
    v = [ctypes.c_int(-1) for _ in range(6)]
    taken = _lib.load().gdmcf_debug_dr_tn_plan(B, N, K, lddz or N, lda or K, ldw or K, bias_col, fused, *[ctypes.byref(x) for x in v])
    return (taken,) + tuple(x.value for x in v)


def test_plan_model_equals_the_library_for_every_batch():
    for fused in (0, 1):
        for B in range(128, 1101):
            Dp, ksp, waste, rounds, stream = D.dr_tn_plan(B)
            assert lib_plan(B, fused=fused) == (1, Dp, ksp, 16, 32, 1, 0), (B, fused)
            assert ksp - D.cdiv(B, 4) == waste and ksp == rounds * (Dp + 1) and stream == (rounds >= D.STREAM_ROUNDS), B
    assert lib_plan(127)[0] == 0 and lib_plan(127) == (0,) * 7
    assert lib_plan(128, K=1984)[0] == 0  # 16 x 31 = 496 tiles


def test_case_table_is_what_the_plan_says():
    assert len(D.CASES) == 12
    for B, (Dp, ksp, waste, rounds, tail) in D.CASES.items():
        assert D.dr_tn_plan(B) == (Dp, ksp, waste, rounds, rounds >= 9), B
        assert B % 4 == tail, B
        assert lib_plan(B)[1:3] == (Dp, ksp), B


def test_case_table_covers_every_configuration():
    plans = {B: D.dr_tn_plan(B) for B in D.CASES}
    modes = {(p[0], p[4]) for p in plans.values()}
    assert modes == {(d, s) for d in (7, 8, 9) for s in (False, True)}  # every depth, stream and spot
    for d in (8, 9):  # both sides of the boundary: 8 rounds (spot), exactly 9 (the 16th row group is consumed in the last round), more
        rounds = {p[3] for p in plans.values() if p[0] == d}
        assert {8, 9} <= rounds and max(rounds) > 9, (d, rounds)
    for stream in (False, True):
        assert any(p[2] > 0 for p in plans.values() if p[4] == stream)  # padded steps
        assert any(B % 4 for B, p in plans.items() if p[4] == stream)   # a partial last k-step
        assert any(p[2] > 0 and B % 4 for B, p in plans.items() if p[4] == stream)  # both at once


def test_depth_seven_never_runs_exactly_nine_rounds():
    """9 rounds of 8 steps are 72 steps, which a ring of 9 slots (D = 8) runs without waste too: ties go to the deeper ring"""
    for B in range(128, 20000):
        Dp, _, _, rounds, _ = D.dr_tn_plan(B)
        assert not (Dp == 7 and rounds == 9), B


def test_plan_reports_tiles_ticket_order_and_bias_column():
    assert lib_plan(321, N=2048, K=1024)[3:6] == (32, 16, 0)            # more row tiles than column tiles: !m_fastest
    assert lib_plan(321, N=2048, K=1024, lda=1032, bias_col=1) == (1, 8, 81, 32, 17, 0, 1)
    assert lib_plan(321, N=1024, K=2048, lda=2056, bias_col=1) == (1, 8, 81, 16, 33, 1, 1)  # the bias column alone in a new column tile
    assert lib_plan(321, N=1024, K=2048, lda=2048, bias_col=1)[6] == 0  # no room for the column: not carried
    assert lib_plan(130, N=64, K=32768)[3:6] == (1, 512, 1)
    assert lib_plan(130, N=100, K=16400)[3:6] == (2, 257, 1)
    assert lib_plan(130, N=1000, K=2100, ldw=2131)[3:5] == (16, 33)
    assert lib_plan(130, N=1024, K=2048, ldw=2047)[0] == 0              # ldw < K


# ---- the product bound -----------------------------------------------------------------------------------------------------------
SUB_N, SUB_K = 48, 80  # the corner of dW the float32 emulation evaluates (every element passes through the same operations)


@pytest.mark.parametrize("B", sorted(D.CASES))
def test_bound_passes_the_kernels_order_in_float32_and_fails_planted_errors(B):
    dZ, A, _ = D.dw_operands(B, N_SWEEP, K_SWEEP)
    dZ, A = dZ[:, :SUB_N], A[:, :SUB_K]
    ref, absprod = D.product_ref(dZ, A)
    bound = D.product_bound(B, absprod)
    got = D.chained_f32(dZ, A)
    assert got.dtype == np.float32
    ratio = D.worst_ratio(got, ref, bound)
    print(f"B = {B}: float32 in the kernels' order reaches {ratio:.4f} of the bound")
    assert ratio <= 1.0
    # one term dropped (a k-step's lane that read zero) and one counted twice: most elements leave the bound, the typical term
    # being sum |terms| / B against a bound of (B + 8) u sum |terms|
    k0 = B - 1
    term = np.outer(dZ[k0].astype(np.float64), A[k0].astype(np.float64))
    for planted in (got.astype(np.float64) - term, got.astype(np.float64) + term):
        over = np.abs(planted - ref) > bound
        assert D.worst_ratio(planted, ref, bound) > 1.0 and over.mean() > 0.9, (B, over.mean())
    # a row that holds its neighbour's values
    moved = np.roll(got, 1, axis=0)
    assert (np.abs(moved.astype(np.float64) - ref) > bound).mean() > 0.99
    # and a NaN is no pass
    got[3, 5] = np.nan
    assert D.worst_ratio(got, ref, bound) == float("inf")


def test_kn_plan_of_the_gpu_cases():
    """the split counts tests/test_gpu_dr_edges.py expects at 256 compute units, from gd_dr_kn_splits / gd_dr_kn_launch by hand"""
    assert D.kn_plan(75, 4100, 128, 256) == (26, 10, 32)   # 257 chunks: 25 splits of 10 and one of 7 (odd: the pair loop ends past it)
    assert D.kn_plan(80, 4096, 120, 256) == (32, 8, 32)
    assert D.kn_plan(150, 5000, 250, 256) == (32, 10, 39)  # 4 tiles, 313 chunks: 39 splits asked, 31 of 10 chunks and one of 3
    assert D.kn_plan(152, 4111, 256, 256) == (26, 10, 32)  # 4 tiles, 257 chunks
    assert D.kn_plan(80, 4080, 128, 256) is None
