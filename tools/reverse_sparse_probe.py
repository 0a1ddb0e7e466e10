"""The reverse loop (p_sample, sampling_steps = 0) on dense rows vs device CSR rows, back to back in one process (bench.py times
the training step; this probe is how the evaluation loop's sparse route is measured).

    python tools/reverse_sparse_probe.py [--iters 10] [--warmup 2] [--rounds 5] [--out profiles/reverse_sparse_probe_yelp.json]

Yelp shape (34 395 items, hid 1000, batch 400, T = 5), f32, eval mode, steps = 0, no sampling noise.  After the same untimed clock
pre-heat as bench.py (clock_preheat), each backbone alternates the two legs on the same model for `rounds` rounds:
  dense:  DeviceCSR.rows(ids) (densify launch) -> p_sample: T hidden products on the dense x_t (one-hot family: the [B, 2I] image,
          and per step both input builders and both branches' products);
  sparse: DeviceCSR.batch(ids) -> p_sample: the first step's first layer is gdmcf_gather_fwd_f32 on the rows' weight rows (one-hot
          family: branch 2's product gathered once per loop, its per-step layer from that sum; no image, no xin2).
Every leg runs `warmup` untimed loops then `iters` timed ones.  Prints one JSON document; ms per loop is the median over the
rounds, *_legs_ms every round, *_spread_ms = max - min of the rounds (the noise a difference has to exceed).  --legs sparse (or
dense) runs one leg alone: a per-kernel profile of it, or the dense loop of another checkout as an anchor."""
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default="dnn,onehot,onehot-emb")
    ap.add_argument("--legs", default="dense,sparse", help="legs to run (one of them alone: per-kernel profiles, anchors)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd.data_utils import DeviceCSR

    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, hid, T, n_pool = 400, 1000, 5, 4
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_pool * B, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    dcsr = DeviceCSR(sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_pool * B, I)), dev)
    row_ids = [torch.arange(i * B, (i + 1) * B, device=dev) for i in range(n_pool)]
    x_buf = torch.empty(B, I, dtype=torch.float32, device=dev)
    sparse_batches = [dcsr.batch(r) for r in row_ids]
    rows_of = {"dense": lambda i: dcsr.rows(row_ids[i], out=x_buf), "sparse": lambda i: sparse_batches[i]}
    legs_wanted = args.legs.split(",")
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per reverse loop (p_sample, steps = 0, T = 5, no sampling noise), dense rows vs device CSR rows, Yelp "
                    "shape, f32, batch 400, eval mode; median over rounds of alternating legs",
               config=dict(n_items=I, n_users=U, hidden=hid, batch=B, T=T, iters=args.iters, warmup=args.warmup,
                           rounds=args.rounds, nnz_per_row=round(len(indices) / (n_pool * B), 2),
                           device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, backbones={})
    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        if backbone == "dnn":
            model = gdmcf_amd.DNN([I, hid], [hid, I], 10, time_type="cat", norm=False)
            diffusion = gdmcf_amd.GaussianDiffusion(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T, dev)
        else:
            if backbone == "onehot":
                model = gdmcf_amd.DNNOneHot([I, hid], [hid, I], 10, time_type="cat", norm=False)
            else:
                model = gdmcf_amd.DNNOneHotEmbedding([I, hid], [hid, I], 10, time_type="cat", norm=False, item_num=I, user_num=U)
            diffusion = gdmcf_amd.GaussianDiffusionDiscrete(gdmcf_amd.ModelMeanType.START_X, "linear-var", 0.01, 0.001, 0.01, T,
                                                            dev, CatOneHot=True)
            diffusion.indexIn = backbone == "onehot-emb"
        model = model.to(dev).eval()
        kw = [dict(index=r) if backbone == "onehot-emb" else {} for r in row_ids]
        legs = {r: [] for r in legs_wanted}
        pred = {}
        for _ in range(args.rounds):
            for leg in legs_wanted:
                rows = rows_of[leg]
                for i in range(args.warmup):  # (the first warm-up loop also builds the cached tables of the weights)
                    diffusion.p_sample(model, rows(i % n_pool), 0, False, **kw[i % n_pool])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.iters):
                    pred[leg] = diffusion.p_sample(model, rows(i % n_pool), 0, False, **kw[i % n_pool])
                torch.cuda.synchronize()
                legs[leg].append(1e3 * (time.perf_counter() - t0) / args.iters)
        res = {}
        for leg in legs_wanted:
            res[f"{leg}_ms_per_loop"] = round(statistics.median(legs[leg]), 4)
            res[f"{leg}_legs_ms"] = [round(v, 4) for v in legs[leg]]
            res[f"{leg}_spread_ms"] = round(max(legs[leg]) - min(legs[leg]), 4)
        if "dense" in legs and "sparse" in legs:
            d, c = res["dense_ms_per_loop"], res["sparse_ms_per_loop"]
            res.update(saved_ms=round(d - c, 4), saved_frac=round((d - c) / d, 4),
                       exceeds_spread=bool(d - c > max(res["dense_spread_ms"], res["sparse_spread_ms"])),
                       max_abs_diff=float((pred["dense"] - pred["sparse"]).abs().max()),
                       max_abs_pred=float(pred["dense"].abs().max()))
        out["backbones"][backbone] = res
        del model, diffusion
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
