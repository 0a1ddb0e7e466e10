"""One LightGCN BPR training step, the autograd route against the fused one, back to back in one process.

    python tools/bpr_step_probe.py [--steps 50] [--warmup 5] [--rounds 5] [--out profiles/bpr_step_probe_yelp.json]
    python tools/bpr_step_probe.py --legs fused_device_sampler --n-negs 1,4,1,4 --neg-pool 1,1,8,8    # the sampler's knobs

Yelp shape (54 574 users, 34 395 items, d = 64, 3 layers, batch 1024, decay 1e-4, lr 0.005).  After the same untimed clock
pre-heat as bench.py, the legs alternate on ONE model for `rounds` rounds, each leg `warmup` untimed steps then `steps` timed
ones between two device synchronisations:
  autograd_presampled   the step exactly as bench.py:bench_bpr runs it: four batches drawn by sample_bpr_batch beforehand,
                        LightGCN.forward + bpr_loss + backward + torch.optim.Adam
  autograd_host_sampler the same with sample_bpr_batch (numpy, host) and the three host-to-device copies inside the loop
  fused_presampled      BPRTrainer.step(u, p, n) on the same four device batches
  fused_device_sampler  BPRTrainer.step(): users by a device generator, items by gdmcf_bpr_sample_f32
  fused_memset          fused_presampled with the cotangent table zeroed by a memset every step (BPRTrainer._memset_G) instead of the
                        regulariser pass clearing the rows the scatter wrote (the product path, the other fused legs)
  fused_device_sampler_n<N>_p<P>   the same from a BPRTrainer(n_negs=N, neg_pool=P): one leg per pair of --n-negs / --neg-pool
                        (comma-separated lists of equal length; the pair 1, 1 is fused_device_sampler itself).  Each such leg
                        also reports the bytes its step gathers, B * n_negs * (1 + pool) * 4 d.
ms per step = median over the rounds; *_legs_ms every round; *_spread_ms = max - min of the rounds, the noise a difference has
to exceed; *_host_enqueue_ms: host time until the last step is enqueued.  --legs runs a subset (one leg alone: the program to
put under rocprofv3 --kernel-trace --stats); --stats-csv FILE --stats-steps N condenses that run's kernel_stats.csv into
per-step figures, N = the steps the traced run took = rounds x (warmup + steps)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("autograd_presampled", "autograd_host_sampler", "fused_presampled", "fused_device_sampler", "fused_memset")


def kernel_stats(path, steps, what):
    """rocprofv3's <name>_kernel_stats.csv of a run of `steps` steps -> device time per step and kernel"""
    from profiles.summarize import short
    rows = sorted(csv.DictReader(open(path)), key=lambda r: -float(r["TotalDurationNs"]))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    kernels = {}
    for r in rows:
        if float(r["TotalDurationNs"]) < 0.002 * total:
            continue
        k = kernels.setdefault(short(r["Name"]), dict(calls_per_step=0.0, us_per_step=0.0))  # (template instances share a short name)
        k["calls_per_step"] = round(k["calls_per_step"] + int(r["Calls"]) / steps, 2)
        k["us_per_step"] = round(k["us_per_step"] + float(r["TotalDurationNs"]) / 1e3 / steps, 2)
    for k in kernels.values():
        k["us_per_call"] = round(k["us_per_step"] / k["calls_per_step"], 2) if k["calls_per_step"] else 0.0
    return dict(what=what, steps=steps, launches_per_step=round(sum(int(r["Calls"]) for r in rows) / steps, 1),
                device_us_per_step=round(total / 1e3 / steps, 1), us_per_step=kernels)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--n-negs", default="1", help="negatives per positive, one value per configuration (comma-separated)")
    ap.add_argument("--neg-pool", default="1", help="candidates per negative, one value per configuration (comma-separated)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats-csv", default=None, help="condense a rocprofv3 kernel_stats.csv (of --stats-steps steps) and exit")
    ap.add_argument("--stats-steps", type=int, default=0)
    args = ap.parse_args(argv)

    if args.stats_csv:
        if args.stats_steps <= 0:
            ap.error("--stats-csv needs --stats-steps: the steps the traced run took, rounds x (warmup + steps)")
        text = json.dumps(kernel_stats(args.stats_csv, args.stats_steps,
                                       "device time per BPRTrainer.step(u, p, n) and kernel (us), Yelp shape, d 64, 3 layers, batch "
                                       "1024: tools/bpr_step_probe.py --legs fused_presampled --rounds 1 --preheat-seconds 0 under rocprofv3 "
                                       "--kernel-trace --stats, totals / steps run (warm-up included); kernels under 0.2 % left out"),
                          indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return

    import scipy.sparse as sp

    import gdmcf_amd
    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd.lightgcn import BPRTrainer, bpr_loss, sample_bpr_batch

    dev = torch.device("cuda:0")
    lib = _lib.load()
    layers, d, B, decay, lr = 3, 64, 1024, 1e-4, 0.005
    cfg = data.SHAPES["yelp"]
    indptr, indices, I = data.synth_csr("yelp", seed=0)
    U = cfg["n_users"]
    users = np.repeat(np.arange(U), np.diff(indptr))
    torch.manual_seed(0)
    m = gdmcf_amd.LightGCN({"user_id_idx": users, "item_id_idx": indices}, U, I, layers, d, device=dev).to(dev)
    R = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(U, I))
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    trainers = {"rows": BPRTrainer(m, R, batch_size=B, lr=lr, decay=decay), "memset": BPRTrainer(m, R, batch_size=B, lr=lr, decay=decay)}
    trainers["memset"]._memset_G = True
    rng = np.random.default_rng(0)
    batches = [[torch.from_numpy(a).to(dev) for a in sample_bpr_batch(indptr, indices, U, I, B, rng)] for _ in range(4)]

    def autograd_step(bu, bp, bn):
        opt.zero_grad()
        out = m(bu, bp, bn)
        mf, reg = bpr_loss(bu, *out)
        (mf + decay * reg).backward()
        opt.step()
        return mf

    def host_sampled(i):
        return autograd_step(*[torch.from_numpy(a).to(dev) for a in sample_bpr_batch(indptr, indices, U, I, B, rng)])

    step_of = {"autograd_presampled": lambda i: autograd_step(*batches[i % 4]),
               "autograd_host_sampler": host_sampled,
               "fused_presampled": lambda i: trainers["rows"].step(*batches[i % 4])[0],
               "fused_device_sampler": lambda i: trainers["rows"].step()[0],
               "fused_memset": lambda i: trainers["memset"].step(*batches[i % 4])[0]}
    legs_run = [leg for leg in args.legs.split(",") if leg]
    knobs = list(zip([int(v) for v in args.n_negs.split(",")], [int(v) for v in args.neg_pool.split(",")]))
    if len(args.n_negs.split(",")) != len(args.neg_pool.split(",")):
        ap.error("--n-negs and --neg-pool take lists of one length")
    gathered = {}
    for n, p in (knobs if knobs != [(1, 1)] else []):
        if (n, p) == (1, 1):
            leg = "fused_device_sampler"
        else:
            leg = f"fused_device_sampler_n{n}_p{p}"
            trainers[leg] = BPRTrainer(m, R, batch_size=B, lr=lr, decay=decay, n_negs=n, neg_pool=p)
            step_of[leg] = lambda i, t=trainers[leg]: t.step()[0]
        gathered[leg] = B * n * (1 + p) * 4 * d
        if leg not in legs_run:
            legs_run.append(leg)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    legs, host, loss = {k: [] for k in legs_run}, {k: [] for k in legs_run}, {}
    for _ in range(args.rounds):
        for leg in legs_run:
            step = step_of[leg]
            for i in range(args.warmup):
                step(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                mf = step(i)
            host[leg].append(1e3 * (time.perf_counter() - t0) / args.steps)
            torch.cuda.synchronize()
            legs[leg].append(1e3 * (time.perf_counter() - t0) / args.steps)
            loss[leg] = float(mf)
    res = {}
    for leg in legs_run:
        res[leg] = dict(ms_per_step=round(statistics.median(legs[leg]), 4), legs_ms=[round(v, 4) for v in legs[leg]],
                        spread_ms=round(max(legs[leg]) - min(legs[leg]), 4),
                        host_enqueue_ms_per_step=round(statistics.median(host[leg]), 4), last_mf=round(loss[leg], 6))
        if leg in gathered:
            res[leg]["gathered_bytes_per_step"] = gathered[leg]
    verdict = {}
    for new, old in (("fused_presampled", "autograd_presampled"), ("fused_device_sampler", "autograd_host_sampler"),
                     ("fused_presampled", "fused_memset")):
        if new in res and old in res:
            a, b = res[new], res[old]
            noise = max(a["spread_ms"], b["spread_ms"])
            verdict[f"{new}_vs_{old}"] = dict(saved_ms=round(b["ms_per_step"] - a["ms_per_step"], 4),
                                              speedup=round(b["ms_per_step"] / a["ms_per_step"], 3), spread_ms=noise,
                                              not_slower=a["ms_per_step"] <= b["ms_per_step"] + noise)
    out = dict(what="ms per LightGCN BPR training step, autograd route (LightGCN.forward + bpr_loss + backward + torch.optim.Adam) vs "
                    "BPRTrainer (gdmcf_bpr_* kernels + FusedAdamW), Yelp shape; median over rounds of alternating legs on one model",
               config=dict(n_users=U, n_items=I, nnz=m.nnz, d=d, layers=layers, batch=B, decay=decay, lr=lr, steps=args.steps,
                           warmup=args.warmup, rounds=args.rounds, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, legs=res, comparisons=verdict)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
