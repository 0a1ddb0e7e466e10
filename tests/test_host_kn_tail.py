"""CPU (-m "not gpu"): gdmcf_debug_kn_tail_rides, the host predicate behind gdmcf_linear_bwd_input_tail_f32 -- whether dr_kn_kernel
takes the product C[M, N] with reduction length K and its task list leaves one of the 256 workgroups without work -- on the shapes
tests/test_gpu_kn_tail.py runs, against the plan worked out by hand, and the binding of the entry's struct."""
import ctypes

import pytest

from gdmcf_amd import _lib

def _cu():
    """Compute units the library plans for: the device's, or 256 (MI355X) without one."""
    n_cu = ctypes.c_int(0)
    try:
        _lib.load().gdmcf_device_info(ctypes.byref(n_cu), None, None, 0)
    except Exception:
        pass
    return n_cu.value if n_cu.value > 0 else 256


def _plan(M, N, K, CU):
    """tasks of dr_kn_kernel's launch as gemm_dr_kn.hip plans them (0: not taken), restated."""
    def cdiv(a, b):
        return (a + b - 1) // b
    if M < 16 or N < 64 or K < 4096:
        return 0
    tiles = cdiv(M, 80) * cdiv(N, 128)
    if cdiv(M, 80) * 80 * 100 > M * 112 or cdiv(N, 128) * 128 * 100 > N * 112 or tiles > 4 * CU:
        return 0
    chunks = cdiv(K, 16)
    splits = min(4 * CU // tiles, chunks // 8, 64)
    if splits < 2:
        return 0
    cps = (cdiv(chunks, splits) + 1) & ~1
    return tiles * cdiv(chunks, cps)


@pytest.mark.parametrize("M,N,K,tasks,rides", [
    (80, 128, 4096, 32, 1),      # one tile, 32 splits
    (150, 256, 4200, 108, 1),    # 4 tiles x 27 splits of 10 chunks
    (400, 1000, 8192, 960, 1),   # 40 tiles x 24 splits
    (400, 1000, 34395, 1000, 1),  # the Yelp shape: 40 tiles x 25 splits, six workgroups idle
    (320, 1024, 4096, 1024, 0),  # 32 tiles x 32 splits: every wave slot has a task
    (80, 128, 4000, 0, 0),       # a reduction the route declines
    (80, 128, 4200, 27, 1),      # the training case of the GPU module
])
def test_idle_workgroup_predicate(M, N, K, tasks, rides):
    """(tasks, rides: worked out by hand for 256 compute units; on another device the restated plan alone is the reference)"""
    CU = _cu()
    plan = _plan(M, N, K, CU)
    if CU == 256:
        assert plan == tasks and (tasks > 0 and (tasks + 3) // 4 < CU) == bool(rides)
    assert _lib.load().gdmcf_debug_kn_tail_rides(M, N, K) == int(plan > 0 and (plan + 3) // 4 < CU)


def test_tail_struct_is_bound_from_the_header():
    names = [n for n, _ in _lib.GdKnTail._fields_]
    assert names == ["rowpart", "ld_rowpart", "nt", "rowsum", "rowdiv", "alpha", "ts", "weight_t", "pt", "T", "H", "Lt_history",
                     "Lt_count", "update_history", "loss_unscaled", "loss", "gradcoef", "loss_mean", "rowscale_mean", "A", "lda",
                     "rowscale", "Ka", "out", "ldo"]
    assert _lib._SIGNATURES["gdmcf_linear_bwd_input_tail_f32"][1][-2:] == [ctypes.c_void_p, ctypes.c_void_p]
