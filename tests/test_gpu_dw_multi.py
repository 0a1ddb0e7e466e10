"""The fused weight-gradient + AdamW products of a training step issued as ONE launch (gdmcf_linear_bwd_weight_adamw_multi_f32,
the default) against one launch per weight (GDMCF_DW_MULTI=0) and against the separate optimiser pass: bit-identical losses,
weights, moments and biases after the same steps -- eager, replayed from a hipGraph, and at a batch too short for the optimiser
stream (every tile updated on the spot)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gdmcf_amd
from gdmcf_amd.gaussian_diffusion import ModelMeanType

DEV = torch.device("cuda:0")
U, I, HID, T = 800, 34395, 1000, 5  # the Yelp width: both large weights on the register-streaming kernel


def _setup(fuse):
    import scipy.sparse as sp
    from gdmcf_amd.data_utils import DeviceCSR
    rng = np.random.default_rng(5)
    dense = (rng.random((U, I)) < 0.006).astype(np.float32)
    dcsr = DeviceCSR(sp.csr_matrix(dense), DEV)
    torch.manual_seed(21)
    model = gdmcf_amd.DNN([I, HID], [HID, I], 10).to(DEV).train()
    diff = gdmcf_amd.GaussianDiffusion(ModelMeanType.START_X, "linear-var", 0.1, 0.001, 0.01, T, DEV)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    if fuse:
        opt.fuse_into_backward(model, min_numel=1 << 12)
    return dcsr, model, diff, opt


def _state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        out += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return out


def _run(monkeypatch, mode, B, steps, graphed=False):
    from gdmcf_amd.parallel import DataParallelStep
    monkeypatch.setenv("GDMCF_DW_MULTI", "0" if mode == "single" else "1")
    batches = [torch.from_numpy(np.random.default_rng(100 + k).permutation(U)[:B].astype(np.int64)) for k in range(steps)]
    dcsr, model, diff, opt = _setup(fuse=mode != "separate")
    if graphed:
        from gdmcf_amd.graph import GraphedTrainStep
        with GraphedTrainStep(diff, model, opt, dcsr, B, warmup=2) as gstep:
            losses = [gstep(b).clone() for b in batches]
            assert gstep.graph is not None
    else:
        step = DataParallelStep(diff, model, opt)
        losses = [step(dcsr.batch(b.to(DEV)), True).clone() for b in batches]
    torch.cuda.synchronize()
    out = losses, _state(model, opt)
    del model, opt
    torch.cuda.empty_cache()
    return out


def _assert_same(a, b):
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), ("loss", k, float(x), float(y))
    for k, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), ("state tensor", k, float((x - y).abs().max()))


def test_one_launch_equals_one_per_weight_and_the_separate_pass(monkeypatch):
    multi = _run(monkeypatch, "multi", 400, 5)
    _assert_same(multi, _run(monkeypatch, "single", 400, 5))
    _assert_same(multi, _run(monkeypatch, "separate", 400, 5))


def test_one_launch_replayed_from_a_graph(monkeypatch):
    _assert_same(_run(monkeypatch, "multi", 400, 5, graphed=True), _run(monkeypatch, "single", 400, 5, graphed=True))


def test_one_launch_with_tiles_updated_on_the_spot(monkeypatch):
    """batch 256: a k loop of 8 ring rounds is too short for the optimiser stream, every tile is updated from its accumulators
    (and the output layer's bias column, N % 64 != 0, takes the element-wise path at any batch)"""
    multi = _run(monkeypatch, "multi", 256, 3)
    _assert_same(multi, _run(monkeypatch, "single", 256, 3))
    _assert_same(multi, _run(monkeypatch, "separate", 256, 3))
