"""From "these users and these candidates" to "the best k of them": gdmcf_amd.recommend(candidates=) on its two routes against
recommend() over the whole catalogue, back to back in one process on the same model.

    python tools/candidates_probe.py [--batches 30] [--rounds 5] [--out profiles/candidates_probe_yelp.json]

Yelp shape (34 395 items, hid 1000, T = 5), f32, eval mode, sampling_steps = 0, k = 20; backbones dnn (K = 1000: the operand of
the last product) and onehot-gcn (K = 3000); n = 16 and 400 users per batch; C = 20, 100, 500, 2000 candidates per user; lists of
uniformly random items and of items drawn by popularity without replacement, as a retriever returns them.  The lists live on the
device before the clock starts.  Legs, alternating for `rounds` rounds of `batches` batches each:
  full       recommend(...) without candidates: the item-wide product and the top-k over I (route "latent-csr");
  picked     recommend(candidates=, candidate_route="picked"): the item-wide product, gdmcf_cand_pick_f32, the top-k over C;
  gathered   recommend(candidates=, candidate_route="gathered"): gdmcf_cand_scores_f32, the top-k over C.
Two numbers per leg and round: device_ms per batch between two HIP events, wall_ms per batch by the host's clock with one
synchronisation at the end.  Per case the JSON document holds the median and max - min over the rounds of each, `saved_*` =
picked - gathered and full - gathered, and `shown_*`: whether that difference exceeds the larger of the two spreads.  The
gathered product alone is timed too (the launch repeated on the operands of one batch): `gather_kernel_us`, and `gather_TBps` =
live candidates x K x 4 bytes over that time.  That leg reads the same rows again and again, so it is a hot-cache rate.  What the
launch takes inside a batch, between the reverse loop and the top-k of other users' rows, comes from a kernel trace of a run
without that leg:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/candidates_probe.py --kernel-reps 0 --lists uniform --sizes 400 \
        --candidates 100 --batches 100 --rounds 2        (cand_scores_kernel<4, ..>: dnn, <12, ..>: onehot-gcn)
`inside_rule`: n * C <= I, where "auto" picks "gathered"."""
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
    ap.add_argument("--batches", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default="dnn,onehot-gcn")
    ap.add_argument("--sizes", default="16,400")
    ap.add_argument("--candidates", default="20,100,500,2000")
    ap.add_argument("--lists", default="uniform,popular")
    ap.add_argument("--kernel-reps", type=int, default=20, help="launches of the stand-alone leg per batch of the others (0: no such leg)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd import engine_core as core
    from gdmcf_amd.data_utils import DeviceCSR
    from gdmcf_amd.recommend import candidate_route_of
    from latent_probe import _pair

    dev = torch.device("cuda:0")
    lib = _lib.load()
    hid, T, k, n_rows = 1000, 5, 20, 1600
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_rows, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    train = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_rows, I))
    dcsr = DeviceCSR(train, dev)
    popularity = torch.from_numpy(np.bincount(indices, minlength=I).astype(np.float32) + 1.0).to(dev)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per batch from user ids and C candidates each to the best 20 of them (sampling_steps = 0, T = 5, Yelp shape, "
                    "f32, eval mode): recommend() over the catalogue vs recommend(candidates=) forced \"picked\" and forced "
                    "\"gathered\"; device_ms between HIP events, wall_ms by the host's clock with one synchronisation at the end; "
                    "median and max - min over rounds of alternating legs; the gathered product alone in gather_kernel_us",
               config=dict(n_items=I, n_users=U, pool_rows=n_rows, hidden=hid, T=T, k=k, batches=args.batches, rounds=args.rounds,
                           warmup=args.warmup, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, cases={})
    sizes = [int(s) for s in args.sizes.split(",")]
    widths = [int(s) for s in args.candidates.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)

    def pool_lists(kind, C):
        """[n_rows, C] int64 on the device: one list per user of the pool."""
        if kind == "uniform":
            return torch.randint(0, I, (n_rows, C), generator=gen, device=dev)
        return torch.cat([torch.multinomial(popularity.expand(400, I).contiguous(), C, replacement=False, generator=gen)
                          for _ in range(n_rows // 400)])

    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        model, diffusion, _, _ = _pair(backbone, I, hid, T, U, dev)
        model = model.to(dev).eval()
        for n in sizes:
            per = n_rows // n
            all_ids = torch.from_numpy(np.concatenate([np.arange((b % per) * n, (b % per) * n + n) for b in range(args.batches)]))
            ids_dev = all_ids.to(dev)
            for C in widths:
                for kind in args.lists.split(","):
                    cand = pool_lists(kind, C)[ids_dev]  # row for row of all_ids, on the device
                    lists = {}

                    def leg(route):
                        def run(nb):
                            kw = {} if route == "full" else dict(candidates=cand[:nb * n], candidate_route=route)
                            lists[route] = gdmcf_amd.recommend(diffusion, model, dcsr, all_ids[:nb * n], k, batch_size=n, **kw)[-n:]
                            assert diffusion.last_recommend_route == "latent-csr"
                            assert route == "full" or diffusion.last_candidate_route == route
                        return run

                    def timed(run, nb):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        run(nb)
                        e1.record()
                        torch.cuda.synchronize()
                        return e0.elapsed_time(e1) / nb, 1e3 * (time.perf_counter() - t0) / nb

                    legs = {route: leg(route) for route in ("full", "picked", "gathered")}
                    dev_ms, wall_ms = {name: [] for name in legs}, {name: [] for name in legs}
                    for _ in range(args.rounds):
                        for name, run in legs.items():
                            run(args.warmup)  # (the first one also builds the cached operands of the weights)
                            d, w = timed(run, args.batches)
                            dev_ms[name].append(d)
                            wall_ms[name].append(w)
                    res = dict(inside_rule=candidate_route_of(n, C, I, True) == "gathered")
                    for kind_t, v in (("device", dev_ms), ("wall", wall_ms)):
                        for name in legs:
                            res[f"{name}_{kind_t}_ms"] = round(statistics.median(v[name]), 4)
                            res[f"{name}_{kind_t}_legs_ms"] = [round(t, 4) for t in v[name]]
                            res[f"{name}_{kind_t}_spread_ms"] = round(max(v[name]) - min(v[name]), 4)
                        for base in ("picked", "full"):
                            saved = res[f"{base}_{kind_t}_ms"] - res[f"gathered_{kind_t}_ms"]
                            res[f"saved_vs_{base}_{kind_t}_ms"] = round(saved, 4)
                            res[f"shown_vs_{base}_{kind_t}"] = bool(abs(saved) > max(res[f"{base}_{kind_t}_spread_ms"],
                                                                                     res[f"gathered_{kind_t}_spread_ms"]))
                    res["lists_equal_picked_gathered"] = bool(torch.equal(lists["picked"], lists["gathered"]))
                    if args.kernel_reps <= 0:
                        out["cases"][f"{backbone}/n={n}/C={C}/{kind}"] = res
                        print(f"{backbone}/n={n}/C={C}/{kind}", json.dumps(res), flush=True)
                        continue
                    # the gathered product alone, on the operands the reverse loop of one batch ends at: back-to-back launches on
                    # the same rows, so a hot-cache rate (the launch inside a batch: see the docstring)
                    chunk = ids_dev[:n]
                    index = chunk if getattr(diffusion, "indexIn", False) else None
                    prod = diffusion._latent_sample(model, dcsr.batch(chunk), 0, index, stop=True)
                    scores = torch.empty(n, C, dtype=torch.float32, device=dev)
                    ptrs = (dcsr.indptr.data_ptr(), dcsr.indices.data_ptr(), None, None)
                    cc = cand[:n].contiguous()

                    def kernel(nb):
                        for _ in range(nb):
                            core.cand_scores(lib, prod.A, prod.second, I, prod.K, prod.bias, prod.scale, cc, C, n, C, ptrs, chunk, scores,
                                             _lib.stream_ptr())

                    kernel(args.warmup)
                    us = [1e3 * timed(kernel, args.kernel_reps * args.batches)[0] for _ in range(args.rounds)]
                    live = int(torch.isfinite(scores).sum())
                    res.update(K=int(prod.K), live_candidates=live, gather_kernel_us=round(statistics.median(us), 3),
                               gather_kernel_spread_us=round(max(us) - min(us), 3),
                               gather_TBps=round(live * int(prod.K) * 4 / (statistics.median(us) * 1e-6) / 1e12, 3))
                    out["cases"][f"{backbone}/n={n}/C={C}/{kind}"] = res
                    print(f"{backbone}/n={n}/C={C}/{kind}", json.dumps(res), flush=True)
        del model, diffusion
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
