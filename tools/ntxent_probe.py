"""NT-Xent term of the embedding backbones: torch route vs HIP kernels (ntxent="fused"), back to back in one process.

    python tools/ntxent_probe.py [--steps 20] [--warmup 3] [--rounds 5] [--out profiles/ntxent_probe_yelp.json]

Yelp shape (34 395 items, hid 1000, batch 400, 54 574 users), f32, the step bench.py times (DataParallelStep at N = 1:
densified device CSR rows -> training_losses -> backward -> FusedAdamW.step).  For each backbone and each optimiser mode
(separate AdamW pass / fuse_into_backward) the legs `torch` and `fused` alternate on ONE model and optimiser (the route is
read from `model.ntxent` at every step) for `rounds` rounds, after the same untimed clock pre-heat as bench.py; every leg
runs `warmup` untimed steps, then `steps` timed ones.  Per leg: median and max - min of ms per step over the rounds, and the
host enqueue time per step (wall time of the steps' Python with no trailing synchronise; near the step time when the step
waits for the device somewhere inside, as the torch route's masked_select does).  The project's bar for a route change:
torch - fused must exceed the larger of the two spreads (`bar_met`)."""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default="onehot-emb,onehot-gcn")
    ap.add_argument("--optimizers", default="separate,fused", help="separate AdamW pass and / or fuse_into_backward")
    ap.add_argument("--legs", default="torch,fused", help="NT-Xent routes to run (one of them alone: per-kernel profiles)")
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
    routes = args.legs.split(",")
    out = dict(what="ms per training step, NT-Xent term by the reference's torch expressions under autograd (torch) vs "
                    "gdmcf_ntxent_fwd_f32 / gdmcf_ntxent_bwd_f32 (fused); Yelp shape, f32, batch 400, DataParallelStep at N = 1; "
                    "median and max - min over rounds of alternating legs",
               config=dict(n_items=I, n_users=U, hidden=hid, batch=B, T=T, steps=args.steps, warmup=args.warmup,
                           rounds=args.rounds, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, backbones={})
    for backbone in args.backbones.split(","):
        out["backbones"][backbone] = {}
        for optimizer in args.optimizers.split(","):
            torch.manual_seed(0)
            cls = gdmcf_amd.DNNOneHotEmbedding if backbone == "onehot-emb" else gdmcf_amd.DNNOneHotEmbeddingGCN
            model = cls([I, hid], [hid, I], 10, time_type="cat", norm=False, item_num=I, user_num=U).to(dev).train()
            diffusion = gdmcf_amd.GaussianDiffusionDiscrete(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T,
                                                            dev, CatOneHot=True)
            diffusion.indexIn = True
            opt = gdmcf_amd.FusedAdamW(model.parameters(), lr=1e-5, weight_decay=0.0)
            if optimizer == "fused":
                opt.fuse_into_backward(model)
            torch.manual_seed(1234)
            step = DataParallelStep(diffusion, model, opt)
            kw = [dict(index=r) for r in row_ids]
            legs, host, loss = {r: [] for r in routes}, {r: [] for r in routes}, None
            for _ in range(args.rounds):
                for route in routes:
                    model.ntxent = route
                    for i in range(args.warmup):
                        step(dcsr.rows(row_ids[i % n_pool], out=x_buf), True, **kw[i % n_pool])
                    torch.cuda.synchronize()
                    assert model.engine.last_ntxent_route == route
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        loss = step(dcsr.rows(row_ids[i % n_pool], out=x_buf), True, **kw[i % n_pool])
                    host[route].append(1e3 * (time.perf_counter() - t0) / args.steps)
                    torch.cuda.synchronize()
                    legs[route].append(1e3 * (time.perf_counter() - t0) / args.steps)
            res = {}
            for route in routes:
                res[f"{route}_ms_per_step"] = round(statistics.median(legs[route]), 4)
                res[f"{route}_spread_ms"] = round(max(legs[route]) - min(legs[route]), 4)
                res[f"{route}_legs_ms"] = [round(v, 4) for v in legs[route]]
                res[f"{route}_host_enqueue_ms_per_step"] = round(statistics.median(host[route]), 4)
            if "torch" in legs and "fused" in legs:
                saved = res["torch_ms_per_step"] - res["fused_ms_per_step"]
                res.update(saved_ms=round(saved, 4), bar_ms=max(res["torch_spread_ms"], res["fused_spread_ms"]),
                           bar_met=bool(saved > max(res["torch_spread_ms"], res["fused_spread_ms"])))
            out["backbones"][backbone][optimizer] = dict(res, final_loss=float(loss))
            if optimizer == "fused":
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
