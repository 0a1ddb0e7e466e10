"""From "these users" to "their top-k items": today's best route through the body of driver.evaluate against gdmcf_amd.recommend
(DESIGN 4.10), back to back in one process on the same model.

    python tools/recommend_probe.py [--batches 50] [--rounds 5] [--out profiles/recommend_probe_yelp.json]
    python tools/recommend_probe.py --mean-type eps --backbones dnn,onehot,dnncat    (recommend(latent="extended"))

Yelp shape (34 395 items, hid 1000, T = 5), f32, eval mode, sampling_steps = 0, k = 20, the four backbones that have the latent
loop, at n = 400 and n = 16 users per batch.  Legs, alternating for `rounds` rounds of `batches` batches each:
  evaluate    per batch dcsr.batch(ids) -> p_sample(latent=True) -> evaluate_utils.csr_rows_to_device (scipy slice of the history,
              two host-to-device copies) -> masked_topk;
  recommend   one recommend(...) call over the same ids with batch_size = n (route "latent-csr").
Two numbers per leg and round:
  device_ms   per batch between two HIP events, with nothing on the host between the launches that a launch does not need: the
              evaluate leg's mask pieces are sliced and uploaded before the first event;
  wall_ms     per batch by the host's clock around the loop as a user runs it, one synchronisation at the end: the evaluate
              leg's host slicing shows only here.
Per case the JSON document holds the median and max - min over the rounds of each, `saved_*` = evaluate - recommend, and
`shown_*`: whether that difference exceeds the larger of the two spreads (a row that misses counts as not shown).
With --mean-type eps or the backbone dnncat the recommend leg is recommend(latent="extended") and the evaluate leg is the same
untouched call, which takes the item-space route for these configurations (`evaluate_route` in the document says so)."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default=None)
    ap.add_argument("--sizes", default="400,16")
    ap.add_argument("--mean-type", default="x0", choices=["x0", "eps"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data, evaluate_utils
    from gdmcf_amd.data_utils import DeviceCSR
    from latent_probe import BACKBONES, _pair

    dev = torch.device("cuda:0")
    lib = _lib.load()
    hid, T, k, n_rows = 1000, 5, 20, 1600
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_rows, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    train = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_rows, I))
    dcsr = DeviceCSR(train, dev)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per batch from user ids to their masked top-20 (sampling_steps = 0, T = 5, Yelp shape, f32, eval mode): the "
                    "body of driver.evaluate(sparse=True, latent=True) vs gdmcf_amd.recommend; device_ms between HIP events "
                    "(evaluate's mask pieces uploaded beforehand), wall_ms by the host's clock with one synchronisation at the end; "
                    "median and max - min over rounds of alternating legs",
               config=dict(mean_type=args.mean_type, n_items=I, n_users=U, pool_rows=n_rows, hidden=hid, T=T, k=k, batches=args.batches, rounds=args.rounds,
                           warmup=args.warmup, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, cases={})

    for backbone in (args.backbones.split(",") if args.backbones else BACKBONES):
        torch.manual_seed(0)
        model, diffusion, _, _ = _pair(backbone, I, hid, T, U, dev, args.mean_type)
        extended = args.mean_type == "eps" or backbone == "dnncat"
        ekw = dict(latent="extended") if extended else {}
        model = model.to(dev).eval()
        with_index = backbone in ("onehot-emb", "onehot-gcn")
        for n in (int(s) for s in args.sizes.split(",")):
            per = n_rows // n
            host_ids = [np.arange((b % per) * n, (b % per) * n + n) for b in range(args.batches)]
            dev_ids = [torch.from_numpy(r).to(dev) for r in host_ids]
            all_ids = np.concatenate(host_ids)
            pieces = [evaluate_utils.csr_rows_to_device(train, r, dev) for r in host_ids[:per]]
            lists = {}

            def evaluate_leg(nb, sliced):
                for b in range(nb):
                    kw = dict(index=dev_ids[b]) if with_index else {}
                    pred = diffusion.p_sample(model, dcsr.batch(dev_ids[b]), 0, False, latent=True, **kw)
                    ip, ix = pieces[b % per] if sliced else evaluate_utils.csr_rows_to_device(train, host_ids[b], dev)
                    lists["evaluate"] = evaluate_utils.masked_topk(pred, k, ip, ix)
                assert diffusion.last_reverse_route == ("item" if extended else "latent")

            def recommend_leg(nb, sliced):
                lists["recommend"] = gdmcf_amd.recommend(diffusion, model, dcsr, all_ids[:nb * n], k, batch_size=n, **ekw)[-n:]
                assert diffusion.last_recommend_route == "latent-csr"

            def timed(leg, nb, sliced):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                leg(nb, sliced)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / nb, 1e3 * (time.perf_counter() - t0) / nb

            legs = {"evaluate": evaluate_leg, "recommend": recommend_leg}
            dev_ms, wall_ms = {name: [] for name in legs}, {name: [] for name in legs}
            for _ in range(args.rounds):
                for name, leg in legs.items():
                    leg(args.warmup, True)  # (the first one also builds the cached operands of the weights)
                    dev_ms[name].append(timed(leg, args.batches, True)[0])
                    wall_ms[name].append(timed(leg, args.batches, False)[1])
            res = {}
            for kind, v in (("device", dev_ms), ("wall", wall_ms)):
                for name in legs:
                    res[f"{name}_{kind}_ms"] = round(statistics.median(v[name]), 4)
                    res[f"{name}_{kind}_legs_ms"] = [round(t, 4) for t in v[name]]
                    res[f"{name}_{kind}_spread_ms"] = round(max(v[name]) - min(v[name]), 4)
                saved = res[f"evaluate_{kind}_ms"] - res[f"recommend_{kind}_ms"]
                res[f"saved_{kind}_ms"] = round(saved, 4)
                res[f"shown_{kind}"] = bool(saved > max(res[f"evaluate_{kind}_spread_ms"], res[f"recommend_{kind}_spread_ms"]))
            # the two legs rank the same users: share of the evaluate leg's lists that recommend's hold (rounding may swap near-ties)
            a, b = lists["evaluate"].cpu().numpy(), lists["recommend"].cpu().numpy()
            res["list_overlap"] = round(float(np.mean([len(set(x) & set(y)) / k for x, y in zip(a, b)])), 6)
            res["lists_equal"] = bool(np.array_equal(a, b))
            res["evaluate_route"] = "item" if extended else "latent"
            out["cases"][f"{backbone}/n={n}"] = res
            print(f"{backbone}/n={n}", json.dumps(res), flush=True)
        del model, diffusion
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
