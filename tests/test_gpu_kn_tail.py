"""GPU (-m gpu): gdmcf_linear_bwd_input_tail_f32 -- the last layer's input gradient with the step's three small launches (row-partial
reducer, float64 loss tail, row scale) on a workgroup that dr_kn_kernel leaves idle -- through the C ABI, bit for bit against those
three launches on their own (gdmcf_kn_tail_run) followed by gdmcf_linear_bwd_input_f32, and against the host models of
tests/glue_ref.py (row_loss, kernel_mean) and of the reducer's summation order below.  NaN where a kernel must write, canaries
around every output.  Shapes (M x N product, reduction K): one tile with 32 splits, the smallest the route takes; clamped rows with K
no multiple of 16; the workload's tiling of M and N.  The fallbacks (no idle workgroup, route declined, GDMCF_KN_TAIL=0, and in a
process of its own GDMCF_DR_KN=0) give the same bits and the same gdmcf_debug_last_gemm as the plain entry.  Then the host wiring:
five training steps through DataParallelStep with the switch on and off and through GraphedTrainStep, and a deferred forward
followed by p_sample instead of its backward."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gdmcf_amd
from gdmcf_amd import _lib
from gdmcf_amd.gaussian_diffusion import ModelMeanType
from tests import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H = 5, 10
RIDING = [(80, 128, 4096), (150, 256, 4200), (400, 1000, 8192)]
F32 = np.float32


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _ceil(n, q):
    return (n + q - 1) // q * q


class Case:
    """Inputs of one call for the product C[M, N] = dZ[M, K] W[K, N]: made once per shape, never written."""

    def __init__(self, M, N, K, nt, T=T, H=H):
        rng = np.random.default_rng([M, N, K])
        self.M, self.N, self.K, self.nt, self.T, self.H = M, N, K, nt, T, H
        self.lddz, self.ldw, self.ldact, self.ldrp = K + 4, _ceil(N, 4) + 4, N + 3, nt + 3
        self.ldo = _ceil(N + 1, 64)  # room for the scale column
        self.dZ = R.seat(M, K, self.lddz, DEV, rng.standard_normal((M, K)).astype(F32))
        self.W = R.seat(K, N, self.ldw, DEV, (rng.standard_normal((K, N)) * 0.02).astype(F32))
        self.act = R.seat(M, N, self.ldact, DEV, np.tanh(rng.standard_normal((M, N))).astype(F32))
        self.h = R.seat(M, N, self.ldact, DEV, np.tanh(rng.standard_normal((M, N))).astype(F32))
        self.rowpart_host = (rng.random((M, nt)) * 3).astype(F32)
        self.rowpart = R.seat(M, nt, self.ldrp, DEV, self.rowpart_host)
        _, self.rowdiv, self.alpha, self.ts, self.weight, self.pt = R.loss_case(M, T, seed=M + N)
        self.dev = [_dev(x) for x in (self.rowdiv, self.alpha, self.ts, self.weight, self.pt)]
        self.hist0 = rng.random((T, H))
        self.cnt0 = rng.integers(H - 3, H + 1, T).astype(np.int64)  # M / T rows per timestep on top: every FIFO wraps
        self.ws = torch.empty(max(int(_lib.load().gdmcf_linear_ws_bytes(M, K, N)), 256), dtype=torch.uint8, device=DEV)


_CASES = {}


def _case(M, N, K, T=T, H=H):
    if (M, N, K, T, H) not in _CASES:
        _CASES[(M, N, K, T, H)] = Case(M, N, K, {80: 37, 150: 64, 400: 135, 320: 70}[M], T, H)
    return _CASES[(M, N, K, T, H)]


def _run(c, entry, update, alpha):
    """One call of `entry` ("tail": the new entry; "plain": gdmcf_kn_tail_run, then gdmcf_linear_bwd_input_f32) on fresh outputs;
    returns ({name: bytes of the output}, gdmcf_debug_last_gemm)."""
    lib, st = _lib.load(), _lib.stream_ptr()
    M, N, K, T, H = c.M, c.N, c.K, c.T, c.H
    f64 = torch.float64
    outs = dict(dh=R.seat(M, N, N + 5, DEV), rowsum=R.seat(1, M, M, DEV), loss_unscaled=R.seat(1, M, M, DEV, dtype=f64),
                loss=R.seat(1, M, M, DEV, dtype=f64), loss_mean=R.seat(1, 1, 1, DEV, dtype=f64), gradcoef=R.seat(1, M, M, DEV),
                rowscale_mean=R.seat(1, M, M, DEV), hs=R.seat(M, N + 1, c.ldo, DEV),
                Lt_history=R.seat(T, H, H, DEV, c.hist0, dtype=f64), Lt_count=R.seat(1, T, T, DEV, c.cnt0, dtype=torch.int64))
    p = {k: v[1].data_ptr() for k, v in outs.items()}
    rowdiv, al, ts, weight, pt = (t.data_ptr() for t in c.dev)
    job = _lib.GdKnTail(c.rowpart[1].data_ptr(), c.ldrp, c.nt, p["rowsum"], rowdiv, al if alpha else None, ts, weight, pt, T, H,
                        p["Lt_history"], p["Lt_count"], int(update), p["loss_unscaled"], p["loss"], p["gradcoef"], p["loss_mean"],
                        p["rowscale_mean"], c.h[1].data_ptr(), c.ldact, p["rowscale_mean"], N, p["hs"], c.ldo)
    args = (c.dZ[1].data_ptr(), c.lddz, c.W[1].data_ptr(), c.ldw, p["rowscale_mean"], c.act[1].data_ptr(), c.ldact, 1, M, K, N,
            p["dh"], N + 5, c.ws.data_ptr(), c.ws.numel())
    if entry == "tail":
        _lib.check(lib.gdmcf_linear_bwd_input_tail_f32(*args, ctypes.byref(job), st))
    else:
        _lib.check(lib.gdmcf_kn_tail_run(ctypes.byref(job), M, st))
        _lib.check(lib.gdmcf_linear_bwd_input_f32(*args, st))
    torch.cuda.synchronize()
    fam = lib.gdmcf_debug_last_gemm()
    res = {}
    for name, (buf, view) in outs.items():
        rows, width = view.shape
        assert R.canary_intact(buf, rows, width, view.stride(0)), name
        a = view.cpu().numpy()
        assert a.dtype.kind != "f" or not np.isnan(a).any(), name  # every element of every output was written
        res[name] = a.copy()
    return res, fam


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _reduce_model(rowpart):
    """rowsum of gd_rowpart_reduce_rows in its own order, float32: lane l adds columns l, l + 64, ... in turn, then the xor tree."""
    M, nt = rowpart.shape
    s = np.zeros((M, 64), dtype=F32)
    for j0 in range(0, nt, 64):
        w = min(64, nt - j0)
        s[:, :w] = s[:, :w] + rowpart[:, j0:j0 + w]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ o]
    assert s.dtype == F32
    return s[:, 0]


@pytest.mark.parametrize("alpha", [False, True], ids=["noalpha", "alpha"])
@pytest.mark.parametrize("update", [0, 1], ids=["keep", "update"])
@pytest.mark.parametrize("M,N,K", RIDING)
def test_riding_tail_equals_the_stand_alone_launches(M, N, K, update, alpha):
    lib = _lib.load()
    assert lib.gdmcf_debug_kn_tail_rides(M, N, K) == 1
    c = _case(M, N, K)
    got, fam = _run(c, "tail", update, alpha)
    want, fam0 = _run(c, "plain", update, alpha)
    assert fam == fam0 == 5
    _same(got, want)
    # ... and the tail against the host models: the reducer's order, the loss tail operation by operation, the scaled copy
    rowsum = _reduce_model(c.rowpart_host)
    assert np.array_equal(got["rowsum"][0], rowsum)
    lu, loss, gc, rsm = R.row_loss(rowsum, c.rowdiv, c.alpha if alpha else None, c.ts, c.weight, c.pt)
    assert np.array_equal(got["loss_unscaled"][0], lu) and np.array_equal(got["loss"][0], loss)
    assert np.array_equal(got["gradcoef"][0], gc) and np.array_equal(got["rowscale_mean"][0], rsm)
    assert got["loss_mean"][0, 0] == R.kernel_mean(loss)
    h = c.h[1].cpu().numpy()
    assert np.array_equal(got["hs"][:, :N], h * rsm[:, None]) and np.array_equal(got["hs"][:, N], rsm)
    if update:
        assert not np.array_equal(got["Lt_history"], c.hist0) and (got["Lt_count"] == H).all()
    else:
        assert np.array_equal(got["Lt_history"], c.hist0) and np.array_equal(got["Lt_count"][0], c.cnt0)
    ref = rsm.astype(np.float64)[:, None] * (c.dZ[1].cpu().numpy().astype(np.float64) @ c.W[1].cpu().numpy().astype(np.float64))
    ref *= 1 - c.act[1].cpu().numpy().astype(np.float64) ** 2
    assert np.abs(got["dh"] - ref).max() <= 2e-5 * np.abs(ref).max() + 1e-9  # (the product itself: test_gpu_fullsize's bound)


def test_riding_tail_with_the_production_history():
    """T = 1000 steps x H = 10 entries: 88 KB of dynamic LDS on dr_kn_kernel's launch, above the default limit."""
    c = _case(*RIDING[0], T=1000, H=10)
    got, fam = _run(c, "tail", 1, True)
    want, fam0 = _run(c, "plain", 1, True)
    assert fam == fam0 == 5
    _same(got, want)
    assert not np.array_equal(got["Lt_history"], c.hist0)


def test_ten_riding_launches_give_the_same_bits():
    c = _case(*RIDING[1])
    first, _ = _run(c, "tail", 1, True)
    for _ in range(9):
        _same(_run(c, "tail", 1, True)[0], first)


def _fallback_shapes():
    """(M, N, K, family): 32 x 32 = 1 024 tasks leave no workgroup idle; K = 4 000 is a reduction the route declines."""
    return [(320, 1024, 4096, 5), (80, 128, 4000, 1)]


@pytest.mark.parametrize("M,N,K,family", _fallback_shapes())
def test_fallback_shapes_equal_the_plain_entry(M, N, K, family):
    assert _lib.load().gdmcf_debug_kn_tail_rides(M, N, K) == 0
    c = _case(M, N, K)
    got, fam = _run(c, "tail", 1, True)
    want, fam0 = _run(c, "plain", 1, True)
    assert fam == fam0 == family
    _same(got, want)


def test_switched_off_equals_the_plain_entry(monkeypatch):
    c = _case(*RIDING[0])
    monkeypatch.setenv("GDMCF_KN_TAIL", "1")
    on, fam_on = _run(c, "tail", 1, True)
    monkeypatch.setenv("GDMCF_KN_TAIL", "0")
    off, fam_off = _run(c, "tail", 1, True)
    want, fam0 = _run(c, "plain", 1, True)
    assert fam_on == fam_off == fam0 == 5
    _same(off, want)
    _same(on, want)


def _route_off_check():
    """(a process started with GDMCF_DR_KN=0) the entry on a shape that would ride: the LDS-tiled kernel serves it, same bits."""
    c = _case(*RIDING[0])
    got, fam = _run(c, "tail", 1, True)
    want, fam0 = _run(c, "plain", 1, True)
    assert fam == fam0 == 1, (fam, fam0)
    _same(got, want)
    print("KN-OFF-OK")


def test_route_switched_off_equals_the_plain_entry():
    r = subprocess.run([sys.executable, "-c", "import tests.test_gpu_kn_tail as t; t._route_off_check()"], cwd=ROOT,
                       env=dict(os.environ, GDMCF_DR_KN="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "KN-OFF-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- host wiring ------------------------------------------------------------------------------------------------------------------
B_TRAIN, I_TRAIN, HID, USERS, STEPS = 80, 4200, 128, 300, 5


def _setup(fuse):
    import scipy.sparse as sp
    from gdmcf_amd.data_utils import DeviceCSR
    rng = np.random.default_rng(11)
    dense = (rng.random((USERS, I_TRAIN)) < 0.01).astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(dense), torch.device(DEV))
    torch.manual_seed(21)
    model = gdmcf_amd.DNN([I_TRAIN, HID], [HID, I_TRAIN], 10).to(DEV).train()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.1, 0.001, 0.01, T, DEV)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    if fuse:
        opt.fuse_into_backward(model, min_numel=1 << 12)
    return dcsr, model, diff, opt


def _state(model, diff, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        out += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return out + [diff.Lt_history.clone(), diff.Lt_count.clone()]


def _batches():
    return [torch.from_numpy(np.random.default_rng(100 + k).permutation(USERS)[:B_TRAIN].astype(np.int64)) for k in range(STEPS)]


def _train(fuse, graph=False):
    from gdmcf_amd.graph import GraphedTrainStep
    from gdmcf_amd.parallel import DataParallelStep
    dcsr, model, diff, opt = _setup(fuse)
    if graph:
        with GraphedTrainStep(diff, model, opt, dcsr, B_TRAIN, warmup=2) as gstep:
            losses = [gstep(b) for b in _batches()]
            assert gstep.graph is not None and gstep.graph is not False, gstep.capture_error
    else:
        step = DataParallelStep(diff, model, opt)
        losses = [step(dcsr.batch(b.to(DEV)), True).clone() for b in _batches()]
    torch.cuda.synchronize()
    return losses, _state(model, diff, opt)


@pytest.mark.parametrize("fuse", [True, False], ids=["fused", "separate"])
def test_five_training_steps_with_and_without_the_passenger(fuse, monkeypatch):
    assert _lib.load().gdmcf_debug_kn_tail_rides(B_TRAIN, HID, I_TRAIN) == 1
    monkeypatch.setenv("GDMCF_KN_TAIL", "0")
    want_l, want = _train(fuse)
    monkeypatch.setenv("GDMCF_KN_TAIL", "1")
    for graph in (False, True):
        got_l, got = _train(fuse, graph=graph)
        for k, (a, b) in enumerate(zip(want_l, got_l)):
            assert torch.equal(a, b), (graph, k, float(a), float(b))
        for k, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), (graph, k)


def test_deferred_forward_followed_by_p_sample(monkeypatch):
    """The backward never comes: the reverse loop runs the stand-alone tail first, and the loss tensors hold its values."""
    monkeypatch.setenv("GDMCF_KN_TAIL", "1")
    res = []
    for defer in (False, True):
        dcsr, model, diff, opt = _setup(False)
        batch = dcsr.batch(_batches()[0].to(DEV))
        eng = model.engine
        eng.defer_tail = defer
        with torch.no_grad():
            losses = diff.training_losses(model, batch, True)
        eng.defer_tail = False
        assert (eng._pending_tail is not None) == defer
        model.eval()
        with torch.no_grad():
            x0 = diff.p_sample(model, batch.dense(), 0, False)
        assert eng._pending_tail is None
        torch.cuda.synchronize()
        bufs = eng.buffers(B_TRAIN, torch.device(DEV))
        res.append([losses["loss"].clone(), eng.last_loss_mean.clone(), bufs.gradcoef.clone(), bufs.rowscale_mean.clone(),
                    bufs.lu.clone(), diff.Lt_history.clone(), diff.Lt_count.clone(), x0.clone()])
    for k, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b), k
    assert bool(torch.isfinite(res[1][0]).all())
