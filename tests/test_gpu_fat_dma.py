"""GPU (-m gpu): dr_fat_kernel's k loop with the weight's pieces loaded straight into LDS (csrc/gemm_dr_fat.hip, GDMCF_FAT_DMA=1)
against the float64 product AND, bit for bit, against the register-staged loop (GDMCF_FAT_DMA=0) -- through the C entries, as
tests/test_gpu_dr_routes.py.

Both loops issue the same MFMAs on the same operands in the same k order, so every output must be IDENTICAL, not close: the
register-staged side runs once, in a fresh child process (the switch is read once per process) that executes this file as a
script, makes every call of every case and leaves the outputs in a temporary directory.

Shapes are the smallest the kernel takes at 256 CUs (>= 512 tiles, K >= 256: M = 400, N = 13 184, see test_gpu_dr_routes.py):
  K = 256, 264, 280, 296   16 | 16 + a half | 17 + a half | 18 + a half chunks of 16: even and odd counts of whole chunks (the loop
                           evens an odd count out with a chunk in front of its pairs), no masked last chunk and one
  ldw = K + 12, lda = K + 4 with NaN behind the K elements of every row: what the DMA brings in beyond K must be masked
  ldw = K + 1              rows that are not 16-byte aligned: served by the register-staged loop, still dr_fat_kernel (4)
  N = 40 000, K = 256      more than one tile per wave (asserted below from the launcher's own rule): the next tile's first pieces
                           land in the LDS that the epilogue has just staged rows in; called twice with different weights
Entries: the fused loss with a dense and with a bitmap target, the posterior with and without noise (N = 13 184 and 40 000 are
below the posterior's 90 % rule).  Tolerance against float64 as test_gpu_dr_routes.py: 2e-5 of max|ref|, absolute, every element.
"""
import functools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from gdmcf_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, PAD = 400, 32
# name: N, K, lda - K, ldw - K, calls (each with weights of its own)
CASES = {
    "k256": (13184, 256, 0, 0, 1),
    "k264": (13184, 264, 0, 0, 1),
    "k280": (13184, 280, 0, 0, 1),
    "k296": (13184, 296, 0, 0, 1),
    "nan_pad": (13184, 264, 4, 12, 1),
    "unaligned": (13184, 264, 0, 1, 1),
    "rounds": (40000, 256, 0, 0, 2),
}
ENTRIES = ("loss", "loss_bits", "post", "post_noise")
RUNS = [(c, e) for c in CASES for e in ENTRIES if c != "rounds" or e in ("loss", "post_noise")]


def fat_tiles(N, n_cu=256):
    """(tile width in blocks of 16 columns, tiles) by gd_dr_fat_launch's rule: the width whose rounds cost the least matrix time"""
    best, nb, tiles = None, 0, 0
    for c in range(12, 7, -1):
        t = -(-M // 80) * -(-N // (16 * c))
        cost = -(-t // (4 * n_cu)) * c
        if t >= 2 * n_cu and (best is None or cost < best):
            best, nb, tiles = cost, c, t
    return nb, tiles


def _padded(t, extra, fill=float("nan")):
    """t's rows in a wider matrix, `fill` behind them; the view has t's shape"""
    full = torch.full((t.shape[0], t.shape[1] + extra), fill)
    full[:, :t.shape[1]] = t
    return full


@functools.lru_cache(maxsize=2)
def _host(name, call):
    """host inputs of one call of one case"""
    N, K, _, _, _ = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(1000 * sorted(CASES).index(name) + call)
    h = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    alpha = torch.rand(M, generator=g) + 0.5
    tgt = torch.rand(M, N, generator=g) < 0.02
    xt = torch.randn(M, N, generator=g)
    z = torch.randn(M, N, generator=g)
    c1, c2, sg = (torch.rand(M, generator=g) + 0.2 for _ in range(3))
    return dict(h=h, W=W, bias=bias, alpha=alpha, tgt=tgt, xt=xt, z=z, c1=c1, c2=c2, sg=sg)


@functools.lru_cache(maxsize=2)
def _dev(name, call):
    """the same on the device: h and W in their padded leading dimensions, NaN behind every row; the target also as bitmaps"""
    N, K, pa, pw, _ = CASES[name]
    t = _host(name, call)
    nw = (N + 31) // 32
    bits = np.zeros((M, nw * 32), dtype=np.uint32)
    bits[:, :N] = t["tgt"].numpy()
    words = (bits.reshape(M, nw, 32) << np.arange(32, dtype=np.uint32)).sum(2, dtype=np.uint64).astype(np.uint32)
    d = {k: v.float().to(DEV) for k, v in t.items() if k not in ("h", "W")}
    return dict(d, h=_padded(t["h"], pa).to(DEV), W=_padded(t["W"], pw).to(DEV), bits=torch.from_numpy(words.view(np.int32)).to(DEV))


@functools.lru_cache(maxsize=2)
def _ref(name, call):
    """float64 references on the host"""
    t = {k: v.double() for k, v in _host(name, call).items()}
    out = t["h"] @ t["W"].t() + t["bias"]
    diff = t["alpha"][:, None] * out - t["tgt"]
    mean = t["c1"][:, None] * out + t["c2"][:, None] * t["xt"]
    return dict(diff=diff, rowsum=(diff * diff).sum(1), pred=out, x_next=mean, x_next_noise=mean + t["sg"][:, None] * t["z"])


def run(name, entry, call):
    """one call through the C entry: the outputs (with their NaN canaries: PAD columns and one row) on the host, and `kernel`, the
    number of the kernel that served it"""
    lib = _lib.load()
    N, K, pa, pw, _ = CASES[name]
    d = _dev(name, call)
    canary = lambda: torch.full((M + 1, N + PAD), float("nan"), device=DEV)
    s = _lib.stream_ptr()
    if entry in ("loss", "loss_bits"):
        diff, rowsum = canary(), torch.full((M + 1,), float("nan"), device=DEV)
        rowpart = torch.zeros(M * lib.gdmcf_loss_tiles(N), device=DEV)
        if entry == "loss":
            _lib.check(lib.gdmcf_linear_loss_fwd_f32(d["h"].data_ptr(), K + pa, d["W"].data_ptr(), K + pw, d["bias"].data_ptr(),
                                                     d["tgt"].data_ptr(), N, d["alpha"].data_ptr(), M, N, K, None, 0, diff.data_ptr(),
                                                     N + PAD, rowpart.data_ptr(), rowsum.data_ptr(), s))
        else:
            _lib.check(lib.gdmcf_linear_loss_fwd_bits_f32(d["h"].data_ptr(), K + pa, d["W"].data_ptr(), K + pw, d["bias"].data_ptr(),
                                                          d["bits"].data_ptr(), d["bits"].shape[1], d["alpha"].data_ptr(), M, N, K,
                                                          None, 0, diff.data_ptr(), N + PAD, rowpart.data_ptr(), rowsum.data_ptr(), s))
        outs = dict(diff=diff, rowsum=rowsum)
    else:
        xn, pred = canary(), canary()
        noise = entry == "post_noise"
        _lib.check(lib.gdmcf_linear_posterior_fwd_f32(d["h"].data_ptr(), K + pa, d["W"].data_ptr(), K + pw, d["bias"].data_ptr(),
                                                      d["xt"].data_ptr(), N, d["c1"].data_ptr(), d["c2"].data_ptr(), None, None,
                                                      d["sg"].data_ptr() if noise else None, d["z"].data_ptr() if noise else None,
                                                      N if noise else 0, M, N, K, xn.data_ptr(), N + PAD, pred.data_ptr(), N + PAD, s))
        outs = dict(x_next=xn, pred=pred)
    torch.cuda.synchronize()
    return dict({k: v.cpu() for k, v in outs.items()}, kernel=torch.tensor(lib.gdmcf_debug_last_gemm()))


def _file(outdir, name, entry, call):
    return os.path.join(outdir, f"{name}-{entry}-{call}.pt")


@functools.lru_cache(maxsize=None)
def _staged():
    """every call of every case with GDMCF_FAT_DMA=0, made by ONE fresh child process: {(case, entry, call): outputs}"""
    with tempfile.TemporaryDirectory() as outdir:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], env=dict(os.environ, GDMCF_FAT_DMA="0"),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return {(n, e, c): torch.load(_file(outdir, n, e, c)) for n, e in RUNS for c in range(CASES[n][4])}


def _assert_close(got, ref, what):
    """every element, 2e-5 of max|ref| absolute; `ref` is float64 on the host"""
    err = float((got.double() - ref).abs().max())
    tol = 2e-5 * float(ref.abs().max())
    print(f"{what}: max err {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol, (what, err, tol)


def test_rounds_case_gives_more_than_one_tile_per_wave():
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == 256, f"dr_fat_kernel's edge shapes are derived for 256 CUs, this device has {n_cu}"
    nb, tiles = fat_tiles(CASES["rounds"][0])
    assert nb == 8 and tiles == 1565 and tiles > 4 * n_cu  # 1 024 waves, one per SIMD
    nb, tiles = fat_tiles(CASES["k256"][0])
    assert nb >= 8 and 2 * n_cu <= tiles <= 4 * n_cu        # the other cases: taken, one tile per wave at the most


@pytest.mark.parametrize("name,entry", RUNS)
def test_dma_loop_matches_float64_and_the_staged_loop(name, entry):
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu == 256, f"dr_fat_kernel's edge shapes are derived for 256 CUs, this device has {n_cu}"
    N = CASES[name][0]
    for call in range(CASES[name][4]):
        got = run(name, entry, call)
        want = _staged()[(name, entry, call)]
        ref = _ref(name, call)
        assert int(got.pop("kernel")) == 4 and int(want["kernel"]) == 4  # dr_fat_kernel, whichever loop ("unaligned": the staged one in both processes)
        for key, t in got.items():
            body = t[:M, :N] if t.dim() == 2 else t[:M]
            _assert_close(body, ref["x_next_noise" if (key, entry) == ("x_next", "post_noise") else key], f"{name} {entry} {call} {key}")
            assert torch.equal(body, want[key][:M, :N] if t.dim() == 2 else want[key][:M]), (name, entry, call, key)
            assert bool(torch.isnan(t[M:]).all()), (key, "canary row behind M")
            if t.dim() == 2:
                assert bool(torch.isnan(t[:, N:]).all()), (key, "canary columns behind N")


if __name__ == "__main__":  # the child: GDMCF_FAT_DMA comes with the environment
    for n, e in sorted(RUNS, key=lambda ne: sorted(CASES).index(ne[0])):
        for c in range(CASES[n][4]):
            torch.save(run(n, e, c), _file(sys.argv[1], n, e, c))
