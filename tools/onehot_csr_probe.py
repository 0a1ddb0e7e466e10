"""Dense rows vs CSR rows on the one-hot backbones, back to back in one process (bench.py times these backbones on dense rows
only; this probe is how the sparse route is measured).

    python tools/onehot_csr_probe.py [--steps 20] [--warmup 3] [--rounds 4] [--out profiles/onehot_csr_probe.json]

Yelp shape (34 395 items, hid 1000, batch 400, 54 574 users), f32, separate AdamW pass, the step bench.py times
(DataParallelStep at N = 1: device CSR rows -> training_losses -> backward -> FusedAdamW.step).  After the same untimed clock
pre-heat as bench.py (clock_preheat), each backbone alternates the two routes on the same model and optimiser for `rounds`
rounds:
  dense: DeviceCSR.rows(ids) (densify launch) -> gdmcf_onehot_noise_f32 -> two gdmcf_dnn_prep_input_f32 -> dense loss target;
  csr:   DeviceCSR.batch(ids) -> gdmcf_dnn_prep_input_csr_f32 + gdmcf_onehot_prep_input_csr_f32 -> bitmap loss target.
Every leg runs `warmup` untimed steps then `steps` timed ones.  Prints one JSON document; ms per step is the median over the
rounds, *_legs_ms every round, *_spread_ms = max - min of the rounds (the noise a difference has to exceed)
(*_host_enqueue_ms_per_step: host time until the last step is enqueued).  --routes csr (or dense) runs one route alone, for a
per-kernel profile of it."""
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
    ap.add_argument("--routes", default="dense,csr", help="legs to run (one of them alone: per-kernel profiles)")
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
    sparse_batches = [dcsr.batch(r) for r in row_ids]
    rows_of = {"dense": lambda i: dcsr.rows(row_ids[i], out=x_buf), "csr": lambda i: sparse_batches[i]}
    routes = args.routes.split(",")
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per training step, dense rows (densify + one-hot image + two dense input builders) vs CSR rows (two "
                    "CSR-fed input builders, bitmap loss target), Yelp shape, f32, batch 400, separate AdamW pass, "
                    "DataParallelStep at N = 1; median over rounds of alternating legs",
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
        legs = {r: [] for r in routes}
        host = {r: [] for r in routes}
        loss = None
        for _ in range(args.rounds):
            for route in routes:
                rows = rows_of[route]
                for i in range(args.warmup):
                    step(rows(i % n_pool), True, **kw[i % n_pool])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    loss = step(rows(i % n_pool), True, **kw[i % n_pool])
                host[route].append(1e3 * (time.perf_counter() - t0) / args.steps)
                torch.cuda.synchronize()
                legs[route].append(1e3 * (time.perf_counter() - t0) / args.steps)
        res = {}
        for route in routes:
            res[f"{route}_ms_per_step"] = round(statistics.median(legs[route]), 4)
            res[f"{route}_legs_ms"] = [round(v, 4) for v in legs[route]]
            res[f"{route}_spread_ms"] = round(max(legs[route]) - min(legs[route]), 4)
            res[f"{route}_host_enqueue_ms_per_step"] = round(statistics.median(host[route]), 4)
        if "dense" in legs and "csr" in legs:
            d, c = res["dense_ms_per_step"], res["csr_ms_per_step"]
            res.update(saved_ms=round(d - c, 4), saved_frac=round((d - c) / d, 4))
        bufs = model.engine.buffers(B, dev)
        res["one_hot_image_allocated"] = bufs.xU is not None  # False for a csr-only run: the [B, 2I] buffer never exists
        out["backbones"][backbone] = dict(res, final_loss=float(loss))
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
