"""The DNNCat backbone's training step against the same module in eager PyTorch, back to back in one process (bench.py has no
leg for this backbone; this probe is its measurement).

    python tools/dnncat_probe.py [--steps 20] [--warmup 3] [--rounds 5] [--legs hip,eager] [--out profiles/dnncat_probe_yelp.json]
    python tools/dnncat_probe.py --legs hip,hip_csr --rounds 5 --out profiles/dnncat_csr_probe_yelp.json

Yelp shape (34 395 items, hid 1000, batch 400), T = 5, f32, x0 target, separate AdamW pass.  After the same untimed clock
pre-heat as bench.py (clock_preheat) the legs alternate for `rounds` rounds, each `warmup` untimed steps then `steps` timed ones:
  hip:   gdmcf_amd.DNNCat under GaussianDiffusionDiscrete(CatOneHot=True): zero_grad -> training_losses -> mean -> backward ->
         FusedAdamW.step (gdmcf_onehot_noise_f32, gdmcf_cat_prep_input_f32, the dense layers, the dxin product, gdmcf_cat_grad_f32);
  hip_csr: the same model built with csr_rows=True (its own instance, optimiser and diffusion), the same row ids handed over as
         dcsr.batch(ids): gdmcf_cat_prep_input_csr_f32, the bitmap loss epilogue, gdmcf_cat_grad_bits_f32 -- no dense batch, no
         [B, 2I] image (`hip` is fed rows densified outside the timed region, so the difference does not include the densify pass);
  eager: the reference's formulas as torch operations on the same GPU -- q_sample, the [B, I, 3] cat, Linear(3, 1), dropout, the
         MLP, the SNR-weighted row mse, autograd, torch.optim.AdamW.  Its one-hot image comes from the same HIP kernel (the
         reference's per-item multinomial is not what is being compared).
Prints one JSON document: ms per step is the median over the rounds, *_legs_ms every round, *_spread_ms = max - min of the
rounds (the noise a difference has to exceed); one_hot_image_allocated says per HIP leg whether its engine holds the [B, 2I]
buffer.  --legs hip (or hip_csr) runs that leg alone, for a per-kernel profile of it."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class EagerDNNCat(nn.Module):
    """models/DNN.py:180-265 in plain torch (one hidden layer each side, as the probe's shape)."""

    def __init__(self, I, hid, emb):
        super().__init__()
        self.emb = emb
        self.emb_layer = nn.Linear(emb, emb)
        self.cat_layer = nn.Linear(3, 1)
        self.in_layer = nn.Linear(I + emb, hid)
        self.out_layer = nn.Linear(hid, I)
        self.drop = nn.Dropout(0.5)

    def forward(self, x, t, x_U):
        from gdmcf_amd import timestep_embedding
        h = self.cat_layer(torch.cat([x.unsqueeze(-1), x_U], dim=2)).squeeze(-1)
        h = torch.cat([self.drop(h), self.emb_layer(timestep_embedding(t, self.emb))], dim=-1)
        return self.out_layer(torch.tanh(self.in_layer(h)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--legs", default="hip,eager")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import numpy as np
    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd.data_utils import DeviceCSR

    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, hid, T, n_pool, emb = 400, 1000, 5, 4, 10
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_pool * B, seed=0)
    dcsr = DeviceCSR(sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_pool * B, I)), dev)
    id_pool = [torch.arange(i * B, (i + 1) * B, device=dev) for i in range(n_pool)]
    legs_on = args.legs.split(",")
    batches = [dcsr.rows(ids) for ids in id_pool] if set(legs_on) & {"hip", "eager"} else None
    csr_batches = [dcsr.batch(ids) for ids in id_pool]
    preheat = clock_preheat(lib, dev, args.preheat_seconds)

    torch.manual_seed(0)
    model = gdmcf_amd.DNNCat([I, hid], [hid, I], emb).to(dev).train()
    diffusion = gdmcf_amd.GaussianDiffusionDiscrete(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, dev,
                                                    CatOneHot=True)
    opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-5, weight_decay=0.0)
    model_csr = None
    if "hip_csr" in legs_on:
        rng_state = torch.get_rng_state()
        torch.manual_seed(0)
        model_csr = gdmcf_amd.DNNCat([I, hid], [hid, I], emb, csr_rows=True).to(dev).train()
        torch.set_rng_state(rng_state)
        diffusion_csr = gdmcf_amd.GaussianDiffusionDiscrete(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T,
                                                            dev, CatOneHot=True)
        opt_csr = gdmcf_amd.FusedAdamW(model_csr.parameters(), lr=1e-5, weight_decay=0.0)
    eager = EagerDNNCat(I, hid, emb).to(dev).train()
    eopt = torch.optim.AdamW(eager.parameters(), lr=1e-5, weight_decay=0.0)
    ca, cb = diffusion._t32["sqrt_ab"], diffusion._t32["sqrt_1mab"]
    w_x0 = diffusion._weights["x0"].float()

    def hip_step(x):
        opt.zero_grad()
        loss = diffusion.training_losses(model, x, True)["loss"].mean()
        loss.backward()
        opt.step()
        return loss

    def hip_csr_step(x):
        opt_csr.zero_grad()
        loss = diffusion_csr.training_losses(model_csr, x, True)["loss"].mean()
        loss.backward()
        opt_csr.step()
        return loss

    def eager_step(x):
        eopt.zero_grad()
        ts_U = torch.randint(0, T, (B,), device=dev)
        ts = torch.randint(0, T, (B,), device=dev)
        x_U, _ = model.engine.onehot_rows(x, ts_U, None, diffusion.discrete)
        x_t = ca[ts][:, None] * x + cb[ts][:, None] * torch.randn_like(x)
        out = eager(x_t, ts, x_U.view(B, I, 2))
        loss = (w_x0[ts] * ((x - out) ** 2).mean(dim=1)).mean()
        loss.backward()
        eopt.step()
        return loss

    steps_of = {"hip": hip_step, "hip_csr": hip_csr_step, "eager": eager_step}
    legs = {k: [] for k in legs_on}
    last = {}
    for _ in range(args.rounds):
        for leg in legs_on:
            fn, pool = steps_of[leg], (csr_batches if leg == "hip_csr" else batches)
            for i in range(args.warmup):
                fn(pool[i % n_pool])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                last[leg] = fn(pool[i % n_pool])
            torch.cuda.synchronize()
            legs[leg].append(1e3 * (time.perf_counter() - t0) / args.steps)
    res = {}
    for leg in legs_on:
        res[f"{leg}_ms_per_step"] = round(statistics.median(legs[leg]), 4)
        res[f"{leg}_legs_ms"] = [round(v, 4) for v in legs[leg]]
        res[f"{leg}_spread_ms"] = round(max(legs[leg]) - min(legs[leg]), 4)
        res[f"{leg}_final_loss"] = float(last[leg])
    if "hip" in res and "eager" in legs:
        res["eager_over_hip"] = round(res["eager_ms_per_step"] / res["hip_ms_per_step"], 3)
    if "hip" in legs and "hip_csr" in legs:
        res["hip_minus_hip_csr_ms"] = round(res["hip_ms_per_step"] - res["hip_csr_ms_per_step"], 4)
        res["larger_spread_ms"] = max(res["hip_spread_ms"], res["hip_csr_spread_ms"])
        res["difference_exceeds_spread"] = bool(res["hip_minus_hip_csr_ms"] > res["larger_spread_ms"])
    res["one_hot_image_allocated"] = {leg: any(getattr(b, "xU", None) is not None for b in m.engine._bufs.values())
                                      for leg, m in (("hip", model), ("hip_csr", model_csr)) if leg in legs}
    out = dict(what="ms per training step of the DNNCat backbone, Yelp shape, f32, batch 400, T = 5, x0 target, separate AdamW "
                    "pass; legs: hip = dense rows, hip_csr = the same rows as a CsrBatch (csr_rows=True), eager = the same "
                    "module in eager PyTorch; median over rounds of alternating legs",
               config=dict(n_items=I, hidden=hid, batch=B, T=T, steps=args.steps, warmup=args.warmup, rounds=args.rounds,
                           device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, **res)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
