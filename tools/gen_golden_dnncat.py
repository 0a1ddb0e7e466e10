"""Fixtures of the DNNCat backbone, recorded from the real reference (imported from its read-only location the way
oracle/gen_golden.py does; nothing of it is copied):

    python tools/gen_golden_dnncat.py

writes tests/golden/dnncat_train_<case>.npz and dnncat_sample_<case>.npz in the format of gen_train_onehot / gen_sample_onehot
of oracle/gen_golden.py (DNNCat has ONE dropout: `drop_mask`, no `drop_mask_U`).  A train file additionally holds
`g0_f64.cat_layer.*`: the first step again with the model in float64 and the same injected draws -- how far the reference's own
float32 sums for the two cat_layer gradients sit from the truth.  `wide_x0` (I = 4100) keeps the state after the last step
(pN / m / v) in dnncat_train_wide_x0_final.npz: ten copies of its two wide weights do not fit one committed file.
"""
import contextlib
import copy
import io
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gen_golden as G  # noqa: E402  (puts the reference on sys.path; `gd` is its gaussian_diffusion module)
from oracle.gen_golden import OUT, REF, _Args, _Index, _extract, gd, make_rows, npy, sd_np  # noqa: E402

_ns = dict(torch=torch, nn=nn, F=F, np=np, math=math, timestep_embedding=G.ref_timestep_embedding)
(RefDNNCat,) = _extract(f"{REF}/models/DNN.py", ["DNNCat"], _ns)


def _pair(I, dims, T, mean_type, schedule, scale, nmin, nmax, emb=10):
    with contextlib.redirect_stdout(io.StringIO()):
        model = RefDNNCat([I] + dims, dims[::-1] + [I], emb, time_type="cat", norm=False)
        mt = {"x0": gd.ModelMeanType.START_X, "eps": gd.ModelMeanType.EPSILON}[mean_type]
        diff = gd.GaussianDiffusionDiscrete(mt, schedule, scale, nmin, nmax, T, "cpu", discrete=0.99, CatOneHot=True, args=_Args())
    return model, diff


def _f64_first_step(model0, diff0, x, draws, noise, sampled, mask):
    """The first training step once more in float64 with the recorded draws injected; returns cat_layer's two gradients."""
    model, diff = copy.deepcopy(model0).double(), copy.deepcopy(diff0)
    model.emb_layer.register_forward_pre_hook(lambda m, i: (i[0].double(),))  # (the sinusoids are the float32 run's values)
    model.drop.register_forward_hook(lambda m, i, o: i[0] * mask.double() * 2.0)
    it = iter(draws)
    diff.sample_timesteps = lambda *a, **k: next(it)
    diff.sample_discrete_features = lambda probX: sampled.clone()
    orig = gd.th.randn_like
    gd.th.randn_like = lambda t: noise.double()
    try:
        model.train()
        diff.training_losses(model, x.double(), True)["loss"].mean().backward()
    finally:
        gd.th.randn_like = orig
    return {"g0_f64." + k: npy(v.grad) for k, v in model.named_parameters() if k.startswith("cat_layer.")}


def gen_train(name, B, I, dims, T, mean_type, schedule="linear-var", scale=0.01, nmin=0.001, nmax=0.01, n_steps=2, lr=1e-3,
              wd=0.0, seed=0, density=0.1, split_final=False):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 100)
    model, diff = _pair(I, dims, T, mean_type, schedule, scale, nmin, nmax)
    opt = torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=wd)
    out = dict(sd_np(model))
    out["meta"] = np.array([f"{B}|{I}|{','.join(map(str, dims))}|{T}|{mean_type}|{schedule}|{scale}|{nmin}|{nmax}|"
                            f"{n_steps}|{lr}|{wd}|10|0|0.99"])
    model0, diff0 = copy.deepcopy(model), copy.deepcopy(diff)
    cap = {"st": [], "drops": []}
    orig_st, orig_q, orig_sd = diff.sample_timesteps, diff.q_sample, diff.sample_discrete_features

    def st(*a, **k):
        cap["depth"] = cap.get("depth", 0) + 1  # 'importance' falls back to a nested 'uniform' call until the history is full
        t, pt = orig_st(*a, **k)
        cap["depth"] -= 1
        if cap["depth"] == 0:
            cap["st"].append((t.clone(), pt.clone()))
        return t, pt

    def q(x, t, noise=None):
        cap["noise"] = noise.clone()
        r = orig_q(x, t, noise)
        cap["x_t"] = r.clone()
        return r

    def sd(probX):
        cap["probX"] = probX.clone()
        r = orig_sd(probX)
        cap["sampled"] = r.clone()
        return r

    diff.sample_timesteps, diff.q_sample, diff.sample_discrete_features = st, q, sd
    model.drop.register_forward_hook(lambda m, i, o: cap["drops"].append((i[0].clone(), o.clone())))
    model.register_forward_hook(lambda m, i, o: cap.update(model_output=o.clone(), x_tU=i[2].clone()))
    model.train()
    for s in range(n_steps):
        x = make_rows(B, I, density, g)
        cap["st"].clear()
        cap["drops"].clear()
        opt.zero_grad()
        terms = diff.training_losses(model, x, True)
        loss = terms["loss"].mean()
        loss.backward()
        assert len(cap["st"]) == 2 and len(cap["drops"]) == 1
        (din, dout), = cap["drops"]
        # the dropout input always has the cat layer's bias added: no exact zeros, so `dout != 0` IS the keep-mask
        assert bool((din != 0).all()), "a zero in the dropout input makes the keep-mask ambiguous"
        mask = dout != 0
        assert din.shape == (B, I) and torch.equal(dout, din * mask.float() * 2.0)
        p = f"s{s}."
        out[p + "x_start"] = npy(x).astype(np.uint8)
        out[p + "ts_U"] = npy(cap["st"][0][0])
        out[p + "ts"], out[p + "pt"] = npy(cap["st"][1][0]), npy(cap["st"][1][1])
        out[p + "sampled"] = npy(cap["sampled"]).astype(np.uint8)
        out[p + "prob1"] = npy(cap["probX"][..., 1])
        out[p + "x_tU"] = npy(cap["x_tU"]).astype(np.uint8)
        out[p + "noise"] = npy(cap["noise"])
        out[p + "drop_mask"] = npy(mask).astype(np.uint8)
        out[p + "x_t"] = npy(cap["x_t"])
        out[p + "model_output"] = npy(cap["model_output"])
        out[p + "loss_vec"] = npy(terms["loss"])
        out[p + "loss"] = npy(loss)
        if s == 0:
            for k, v in model.named_parameters():
                out["g0." + k] = npy(v.grad)
            out.update(_f64_first_step(model0, diff0, x, [(t.clone(), q_.clone()) for t, q_ in cap["st"]], cap["noise"],
                                       cap["sampled"], mask))
        opt.step()
        out[p + "Lt_history"], out[p + "Lt_count"] = npy(diff.Lt_history), npy(diff.Lt_count)
    final = {}
    for k, v in model.named_parameters():
        final["pN." + k] = npy(v)
        final["m." + k], final["v." + k] = npy(opt.state[v]["exp_avg"]), npy(opt.state[v]["exp_avg_sq"])
    if split_final:
        np.savez_compressed(os.path.join(OUT, f"dnncat_train_{name}_final.npz"), **final)
    else:
        out.update(final)
    np.savez_compressed(os.path.join(OUT, f"dnncat_train_{name}.npz"), **out)
    err = {k: float(np.abs(out["g0." + k].astype(np.float64) - out["g0_f64." + k]).max() / np.abs(out["g0_f64." + k]).max())
           for k in ("cat_layer.weight", "cat_layer.bias")}
    print(f"dnncat_train_{name}: loss0={float(out['s0.loss']):.6g} kept bits {int(out['s0.x_tU'].sum())} "
          f"f32-vs-f64 cat grads {err}")


def gen_sample(name, B, I, dims, T, mean_type, seed=0, density=0.08, scale=0.01, nmin=0.001, nmax=0.01):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 7)
    model, diff = _pair(I, dims, T, mean_type, "linear-var", scale, nmin, nmax)
    with torch.no_grad():
        model.out_layers[-1].bias.normal_(0.0, 0.5, generator=g)
    model.eval()
    x = make_rows(B, I, density, g)
    out = dict(sd_np(model))
    out["meta"] = np.array([f"{B}|{I}|{','.join(map(str, dims))}|{T}|{mean_type}|{scale}|{nmin}|{nmax}|0.99"])
    out["x_start"] = npy(x).astype(np.uint8)
    cap = {"noises": [], "sampled": []}
    orig_randn, orig_sd = gd.th.randn_like, diff.sample_discrete_features

    def rl(t):
        n = orig_randn(t)
        cap["noises"].append(n.clone())
        return n

    def sd(probX):
        r = orig_sd(probX)
        cap["sampled"].append(r.clone())
        return r

    gd.th.randn_like, diff.sample_discrete_features = rl, sd
    try:
        with torch.no_grad():
            out["pred_steps0"] = npy(diff.p_sample(model, x, 0, False, index=_Index()))
            cap["noises"].clear()
            cap["sampled"].clear()
            out["pred_stepsT"] = npy(diff.p_sample(model, x, T, False, index=_Index()))
            out["noise_stepsT"], out["sampled_stepsT"] = npy(cap["noises"][0]), npy(cap["sampled"][0]).astype(np.uint8)
            assert len(cap["noises"]) == 1 and len(cap["sampled"]) == 1 + T  # + one graph draw per reverse step
            cap["noises"].clear()
            cap["sampled"].clear()
            out["pred_noisy"] = npy(diff.p_sample(model, x, 2, True, index=_Index()))
            assert len(cap["noises"]) == 1 + T
            out["noise_noisy0"], out["sampled_noisy0"] = npy(cap["noises"][0]), npy(cap["sampled"][0]).astype(np.uint8)
            out["noise_noisy_steps"] = np.stack([npy(n) for n in cap["noises"][1:]])
    finally:
        gd.th.randn_like = orig_randn
    np.savez_compressed(os.path.join(OUT, f"dnncat_sample_{name}.npz"), **out)
    print(f"dnncat_sample_{name}: |pred0| {np.abs(out['pred_steps0']).mean():.3g}")


def main():
    gen_train("tiny_x0", 8, 64, [16], 5, "x0", seed=61)
    gen_train("ragged_eps_wd", 12, 131, [24], 5, "eps", seed=62, density=0.05, wd=0.01, schedule="linear", scale=0.1)
    gen_train("deep_x0", 10, 90, [32, 16], 5, "x0", seed=63, density=0.06)
    # (B = 3 < T: the reference scales the class noise's level as ts / B (:775) and its multinomial rejects the negative
    # probabilities of ts = 4; seed 66 is the first from 64 whose draws of that timestep stay below 4 in both steps)
    gen_train("wide_x0", 3, 4100, [8], 5, "x0", seed=66, density=0.01, split_final=True)
    gen_sample("tiny_x0", 8, 64, [16], 5, "x0", seed=71)
    gen_sample("ragged_eps", 10, 131, [24], 5, "eps", seed=72, scale=50.0)


if __name__ == "__main__":
    main()
