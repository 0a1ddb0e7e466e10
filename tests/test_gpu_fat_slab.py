"""GPU (-m gpu): the first-layer forward as split-K slabs on dr_fat_kernel's LDS-DMA loop (csrc/gemm_dr_fat.hip:
dr_fat_kernel<NB, GD_EPI_SLAB, 1>, family 6, GDMCF_DR_FAT_SLAB) through gdmcf_linear_fwd_f32, against the float64 host product.

Every call: NaN-filled output (one guard row behind M, guard columns behind N) and NaN-filled workspace, NaN behind the K elements of
every row of A (lda = K + 4) and W (ldw = K + 12) unless a case says otherwise -- the chunk that reaches past K must not let them
in.  Tolerance as tests/test_gpu_fullsize.py and tests/test_gpu_fat_dma.py: every element within 2e-5 of max|ref|, absolute; ref =
tanh(A W^T + b) with act = 1, A W^T with act = 0 and no bias.  Shapes are chosen with gdmcf_debug_fat_slab_plan, the launcher's own
plan, so no CU count is assumed: wherever the plan takes the shape, gdmcf_debug_last_gemm() must say 6.

Weights that are not 16-byte aligned (ldw % 4 != 0, or a base 4 bytes off) are NOT declined: they run the register-staged loop
(DMA = 0) on the same plan, family 6, and must equal the aligned call bit for bit -- tests/test_gpu_dw_multi.py requires a seated
weight (fused optimiser) and a contiguous one (separate optimiser, odd K) to give the same training run bit for bit, which a route
that depended on the weight's alignment could not.  The declines left are K < 4 096, M that pads by more than 12 %, and the switch.

A task of the kernel runs the chunks [c_lo, c_hi) of 16 k of one split: an odd count of whole chunks is evened out by one chunk in
front of the pair loop, the chunk that reaches past K is a body of its own and exists in the last split only -- where it may be
the only chunk.  test_chunk_ranges computes from the plan which of those cases each K hits and fails if one was never run.
"""
import ctypes
import functools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8
NAN = float("nan")


def plan(M, N, K):
    """(taken, nb, splits, cps) of the fat-tile slab route for this product on this device"""
    nb, sp, cps = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    taken = _lib.load().gdmcf_debug_fat_slab_plan(M, N, K, ctypes.byref(nb), ctypes.byref(sp), ctypes.byref(cps))
    return bool(taken), nb.value, sp.value, cps.value


@functools.lru_cache(maxsize=4)
def _host(M, N, K):
    """host operands of one shape and both float64 references: pre-activations of order 1, so that tanh does not hide an error"""
    g = torch.Generator(device="cpu").manual_seed(M * 1000003 + N * 1009 + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * (0.7 / K ** 0.5)
    b = torch.randn(N, generator=g) * 0.3
    lin = A.double() @ W.double().t()
    return A, W, b, lin, torch.tanh(lin + b.double())


def _seat(t, ld, offset=0):
    """t's rows at leading dimension ld in a NaN-filled device buffer that starts `offset` floats behind an aligned base"""
    rows, cols = t.shape
    flat = torch.full((rows * ld + offset + 4,), NAN, device=DEV)
    view = flat[offset:offset + rows * ld].view(rows, ld)
    view[:, :cols] = t.to(DEV)
    return view


def forward(M, N, K, act, lda=None, ldw=None, w_offset=0, repeats=0):
    """One gdmcf_linear_fwd_f32 call: (output with its NaN guards on the host, family code, float64 reference).  repeats > 0: that
    many further launches on the same operands, each compared bit for bit with the first."""
    lib = _lib.load()
    A, W, b, lin, ref = _host(M, N, K)
    lda = K + 4 if lda is None else lda
    ldw = K + 12 if ldw is None else ldw
    dA, dW = _seat(A, lda), _seat(W, ldw, w_offset)
    bias = b.to(DEV) if act else None
    ws = torch.full((int(lib.gdmcf_linear_ws_bytes(M, N, K)) // 4,), NAN, device=DEV)
    out = torch.full((M + 1, N + PAD), NAN, device=DEV)

    def launch(o):
        _lib.check(lib.gdmcf_linear_fwd_f32(dA.data_ptr(), lda, dW.data_ptr(), ldw, _lib.ptr(bias), act, M, N, K, o.data_ptr(), N + PAD,
                                            ws.data_ptr(), ws.numel() * 4, _lib.stream_ptr()))
        torch.cuda.synchronize()

    launch(out)
    family = lib.gdmcf_debug_last_gemm()
    for k in range(repeats):
        again = torch.full_like(out, NAN)
        launch(again)
        assert torch.equal(again[:M, :N], out[:M, :N]), f"launch {k + 2} of ({M}, {N}, {K}) differs from the first"
    return out.cpu(), family, (ref if act else lin)


def check(M, N, K, act, family, what, **kw):
    out, fam, ref = forward(M, N, K, act, **kw)
    assert fam == family, (what, "kernel family", fam, "expected", family)
    err = float((out[:M, :N].double() - ref).abs().max())  # (NaN anywhere inside fails the comparison below)
    tol = 2e-5 * float(ref.abs().max())
    print(f"{what} ({M}, {N}, {K}) act={act}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (what, err, tol)
    assert bool(torch.isnan(out[M:]).all()), (what, "guard row behind M written")
    assert bool(torch.isnan(out[:, N:]).all()), (what, "guard columns behind N written")


def chunk_cases(M, N, K):
    """the chunk-range cases that the tasks of this product run, from the launcher's plan (empty when the route declines)"""
    taken, nb, splits, cps = plan(M, N, K)
    if not taken:
        return set()
    assert splits >= 2 and (splits - 1) * cps < -(-K // 16) <= splits * cps
    whole_last = (K >> 4) - (splits - 1) * cps  # whole chunks of the last split
    assert whole_last >= 0
    cases = {"non-last split: odd count" if cps & 1 else "non-last split: even count", "K % 16 == 0" if K % 16 == 0 else "K % 16 != 0"}
    if K % 16:
        cases.add("last split: only the masked chunk" if whole_last == 0 else "last split: one whole chunk + masked" if whole_last == 1 else
                  "last split: odd whole chunks (>= 3) + masked" if whole_last & 1 else "last split: even whole chunks (>= 2) + masked")
    else:
        cases.add("last split: odd whole chunks, none masked" if whole_last & 1 else "last split: even whole chunks, none masked")
    return cases


ALL_CHUNK_CASES = {"non-last split: odd count", "non-last split: even count", "K % 16 == 0", "K % 16 != 0",
                   "last split: only the masked chunk", "last split: one whole chunk + masked",
                   "last split: odd whole chunks (>= 3) + masked", "last split: even whole chunks (>= 2) + masked",
                   "last split: odd whole chunks, none masked", "last split: even whole chunks, none masked"}


def test_chunk_ranges():
    """tiny products: K from 4 096 upward in steps of 4 (ldw = K + 12 stays a multiple of 4), each K kept that runs a case no
    earlier K has run, until every case has been seen"""
    seen, picked = set(), []
    for K in range(4096, 4096 + 2048, 4):
        new = chunk_cases(80, 144, K) - seen
        if new:
            picked.append(K)
            seen |= new
        if seen == ALL_CHUNK_CASES:
            break
    print("K values:", picked)
    assert seen == ALL_CHUNK_CASES, ("cases never hit", ALL_CHUNK_CASES - seen)
    assert len(picked) <= 12
    for K in picked:
        for N in (144, 150):
            assert plan(80, N, K)[0]
            check(80, N, K, 1, 6, "chunk range")
            check(80, N, K, 0, 6, "chunk range")
        # the same ranges on the register-staged loop (rows of the weight not 16-byte aligned): the aligned call's bits
        aligned, _, _ = forward(80, 144, K, 0)
        staged, fam, _ = forward(80, 144, K, 0, ldw=K + 13)
        assert fam == 6 and torch.equal(aligned[:80, :144], staged[:80, :144]), ("staged loop", K)


@pytest.mark.parametrize("M,N", [(400, 999), (400, 1000), (150, 1000), (150, 999)])
def test_tile_edges(M, N):
    """N = 999: no multiple of 4, the slab rows are round4(N) wide and the last column tile lies partly outside; N = 1 000: the
    column tiles together are wider than N (NB = 9: 7 x 144 = 1 008); M = 150: two row tiles, ten rows of padding that are not
    stored; M = 400: five row tiles.  K = 4 100 has a masked chunk."""
    K = 4100
    taken, nb, splits, cps = plan(M, N, K)
    assert taken and -(-N // (16 * nb)) * 16 * nb > N
    if torch.cuda.get_device_properties(0).multi_processor_count == 256 and M == 400:
        assert nb == 9
    check(M, N, K, 1, 6, "tile edge")
    check(M, N, K, 0, 6, "tile edge")


DECLINES = {
    "K = 4 000": dict(M=80, N=144, K=4000),
    "M = 200: three tiles, 20 % padding": dict(M=200, N=144, K=4100),
}


@pytest.mark.parametrize("name", sorted(DECLINES))
def test_declined_products_run_on_the_lds_tiled_kernel(name):
    kw = dict(DECLINES[name])
    M, N, K = kw.pop("M"), kw.pop("N"), kw.pop("K")
    assert plan(80, 144, 4100)[0]  # (the neighbour that is taken)
    check(M, N, K, 1, 1, name, **kw)
    check(M, N, K, 0, 1, name, **kw)


@pytest.mark.parametrize("M,N,K", [(80, 150, 4100), (80, 144, 4116), (400, 1000, 4228)])
@pytest.mark.parametrize("name,kw", [("ldw % 4 != 0", dict(ldw_extra=13)), ("W base offset by 4 bytes", dict(w_offset=1))])
def test_unaligned_weights_run_the_staged_loop_bit_for_bit(M, N, K, name, kw):
    """family 6 on the register-staged loop: within the tolerance, and every bit of the aligned call's result (same plan, same
    MFMAs, same k order); the three K have an even / odd count of whole chunks per split and a masked last chunk"""
    assert plan(M, N, K)[0]
    kw = dict(kw)
    if "ldw_extra" in kw:
        kw["ldw"] = K + kw.pop("ldw_extra")
    for act in (1, 0):
        check(M, N, K, act, 6, name, **kw)
        aligned, fam, _ = forward(M, N, K, act)
        unaligned, fam_u, _ = forward(M, N, K, act, **kw)
        assert fam == 6 and fam_u == 6
        assert torch.equal(aligned[:M, :N], unaligned[:M, :N]), (name, M, N, K, act)


def test_route_switch_off_in_a_fresh_process():
    """GDMCF_DR_FAT_SLAB=0 (read once per process): the same product on the LDS-tiled kernel, same tolerance"""
    assert plan(80, 144, 4100)[0]
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDMCF_DR_FAT_SLAB="0"), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("M,N,K,lda,ldw", [(400, 1000, 34405, 34432, 34432), (400, 4096, 4096, 4096, 4096)])
def test_shapes_that_ship(M, N, K, lda, ldw):
    """the Yelp first layer with seated rows, and the contiguous product of bench.py's clock pre-heat: every element, then twenty more
    launches bit for bit (a fragment read before its LDS-DMA piece has landed shows as a difference between launches)"""
    assert plan(M, N, K)[0]
    check(M, N, K, 1, 6, "ship", lda=lda, ldw=ldw, repeats=20)
    check(M, N, K, 0, 6, "ship", lda=lda, ldw=ldw)


def _train(graphed, steps=5):
    """five training steps of the default engine at B = 80, I = 4 200, hid = 144: (losses, parameters)"""
    import scipy.sparse as sp

    import gdmcf_amd
    from gdmcf_amd.data_utils import DeviceCSR
    from gdmcf_amd.gaussian_diffusion import ModelMeanType
    from gdmcf_amd.graph import GraphedTrainStep
    from gdmcf_amd.parallel import DataParallelStep
    U, I, hid, B = 200, 4200, 144, 80
    rng = np.random.default_rng(3)
    dcsr = DeviceCSR(sp.csr_matrix((rng.random((U, I)) < 0.01).astype(np.float32)), torch.device(DEV))
    torch.manual_seed(11)
    model = gdmcf_amd.DNN([I, hid], [hid, I], 10).to(DEV).train()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.1, 0.001, 0.01, 5, torch.device(DEV))
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    opt.fuse_into_backward(model, min_numel=1 << 12)
    batches = [torch.from_numpy(np.random.default_rng(50 + k).permutation(U)[:B].astype(np.int64)) for k in range(steps)]
    if graphed:
        with GraphedTrainStep(diff, model, opt, dcsr, B, warmup=2) as gstep:
            losses = [gstep(b).clone() for b in batches]
            assert gstep.graph is not None
    else:
        step = DataParallelStep(diff, model, opt)
        losses = [step(dcsr.batch(b.to(DEV)), True).clone() for b in batches]
    torch.cuda.synchronize()
    return losses, [p.detach().clone() for p in model.parameters()]


def test_training_step_is_deterministic_and_graph_replay_changes_no_bit():
    """the route is static (plan from the shape, fixed slab order): eager twice, and eager against GraphedTrainStep, bit for bit"""
    assert plan(80, 144, 4210)[0]  # the first layer's product: I + the 10 timestep-embedding columns
    runs = [_train(False), _train(False), _train(True)]
    for other, what in ((runs[1], "second eager run"), (runs[2], "graph replay")):
        for k, (a, b) in enumerate(zip(runs[0][0], other[0])):
            assert torch.equal(a, b), (what, "loss of step", k, float(a), float(b))
        for a, b in zip(runs[0][1], other[1]):
            assert torch.equal(a, b), (what, "parameter")


if __name__ == "__main__":  # the child of test_route_switch_off_in_a_fresh_process: GDMCF_DR_FAT_SLAB=0 comes with the environment
    assert not plan(80, 144, 4100)[0]
    check(80, 144, 4100, 1, 1, "route off")
    check(80, 144, 4100, 0, 1, "route off")
