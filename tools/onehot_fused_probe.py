"""Separate vs fused AdamW on the one-hot backbones, back to back in one process (bench.py refuses --backbone onehot*
--fuse-optimizer; this probe is how that combination is measured).

    python tools/onehot_fused_probe.py [--steps 20] [--warmup 3] [--rounds 4] [--out profiles/onehot_fused_probe.json]

Yelp shape (34 395 items, hid 1000, batch 400, 54 574 users), f32, the step bench.py times (DataParallelStep at N = 1:
densified device CSR rows -> training_losses -> backward -> FusedAdamW.step).  After the same untimed clock pre-heat as
bench.py (clock_preheat), each backbone alternates the separate pass and the fused one (fuse_into_backward / unfuse on the
same model and optimiser) for `rounds` rounds; every leg runs `warmup` untimed steps then `steps` timed ones.  Prints one
JSON document; ms per step is the median over the rounds
(*_host_enqueue_ms_per_step: host time until the last step is enqueued; near the step time when the step waits for the
device somewhere inside)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default="onehot,onehot-emb,onehot-gcn")
    ap.add_argument("--modes", default="separate,fused", help="legs to run (one of them alone: per-kernel profiles)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd.data_utils import DeviceCSR
    from gdmcf_amd.parallel import DataParallelStep

    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, hid, T, n_pool = 400, 1000, 5, 4
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_pool * B, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    dcsr = DeviceCSR(sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_pool * B, I)), dev)
    row_ids = [torch.arange(i * B, (i + 1) * B, device=dev) for i in range(n_pool)]
    x_buf = torch.empty(B, I, dtype=torch.float32, device=dev)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per training step, separate AdamW pass vs AdamW fused into the backward (FusedAdamW.fuse_into_backward), "
                    "Yelp shape, f32, batch 400, DataParallelStep at N = 1; median over rounds of alternating legs",
               config=dict(n_items=I, n_users=U, hidden=hid, batch=B, T=T, steps=args.steps, warmup=args.warmup,
                           rounds=args.rounds, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, backbones={})
    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        if backbone == "onehot":
            model = gdmcf_amd.DNNOneHot([I, hid], [hid, I], 10, time_type="cat", norm=False)
        else:
            cls = gdmcf_amd.DNNOneHotEmbedding if backbone == "onehot-emb" else gdmcf_amd.DNNOneHotEmbeddingGCN
            model = cls([I, hid], [hid, I], 10, time_type="cat", norm=False, item_num=I, user_num=U)
        model = model.to(dev).train()
        diffusion = gdmcf_amd.GaussianDiffusionDiscrete(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T,
                                                        dev, CatOneHot=True)
        diffusion.indexIn = backbone != "onehot"
        opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-5, weight_decay=0.0)
        torch.manual_seed(1234)
        step = DataParallelStep(diffusion, model, opt)
        kw = [dict(index=r) if backbone != "onehot" else {} for r in row_ids]
        legs = {"separate": [], "fused": []}
        host = {"separate": [], "fused": []}
        loss = None
        for _ in range(args.rounds):
            for mode in args.modes.split(","):
                if mode == "fused":
                    opt.fuse_into_backward(model)
                else:
                    opt.unfuse(model)
                for i in range(args.warmup):
                    step(dcsr.rows(row_ids[i % n_pool], out=x_buf), True, **kw[i % n_pool])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    loss = step(dcsr.rows(row_ids[i % n_pool], out=x_buf), True, **kw[i % n_pool])
                host[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
                torch.cuda.synchronize()
                legs[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
        fused_params = sorted(k for k, p in model.named_parameters() if id(p) in opt._fused_ids)
        res = {}
        for mode in ("separate", "fused"):
            if legs[mode]:
                res[f"{mode}_ms_per_step"] = round(statistics.median(legs[mode]), 4)
                res[f"{mode}_legs_ms"] = [round(v, 4) for v in legs[mode]]
                res[f"{mode}_host_enqueue_ms_per_step"] = round(statistics.median(host[mode]), 4)
        if legs["separate"] and legs["fused"]:
            sep, fus = res["separate_ms_per_step"], res["fused_ms_per_step"]
            res.update(saved_ms=round(sep - fus, 4), saved_frac=round((sep - fus) / sep, 4))
        out["backbones"][backbone] = dict(res, fused_params=fused_params, final_loss=float(loss))
        opt.unfuse(model)
        del model, opt, step, diffusion
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
