"""The rank launch next to the top-k launch on the same scores, and driver.evaluate(recommend=True) with and without ranks=True
(DESIGN 4.12), back to back in one process.

    python tools/rank_probe.py [--reps 50] [--rounds 5] [--out profiles/rank_probe_yelp.json]
    python tools/rank_probe.py --long-row 0      (without the one long row, whose workgroup sets the launch's latency)

Yelp shape (34 395 items), [n, I] float32 scores, the history mask picked by user id, n = 400 and n = 16 rows.  Targets: about 10
per user and one row of 1000.  Legs, alternating for `rounds` rounds of `reps` launches each, timed between two HIP events:
  rank       gdmcf_rank_targets_f32 (ranks and n_live)
  topk20     gdmcf_topk_masked_rows_f32, k = 20
  topk100    gdmcf_topk_masked_rows_f32, k = 100
All three read the n x I scores once: `score_gbs` is 4 n I bytes over the launch's time, to be held against what
tools/hbm_peak.py reports for a read on the same box (at n = 16 the scores fit the caches: a launch's latency, not a rate).
Per leg the JSON document holds the median and max - min over the rounds.  The second part times driver.evaluate(recommend=True)
on `--eval-users` users of the DNN backbone (hid 1000, T = 5) with and without ranks=True by the host's clock (the call ends in
the copy of its per-user terms), alternating, and checks that both return the same metrics."""
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--sizes", default="400,16")
    ap.add_argument("--eval-users", type=int, default=1600)
    ap.add_argument("--long-row", type=int, default=1000, help="targets of the one long row (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    from bench import clock_preheat
    from gdmcf_amd import _lib, data, driver
    from gdmcf_amd.data_utils import DeviceCSR
    from latent_probe import _pair

    dev = torch.device("cuda:0")
    lib = _lib.load()
    n_rows = max(1600, args.eval_users)
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_rows, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    train = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_rows, I))
    rng = np.random.default_rng(1)
    per_user = [rng.choice(I, size=int(c), replace=False) for c in rng.integers(5, 16, n_rows)]
    if args.long_row:
        per_user[7] = rng.choice(I, size=args.long_row, replace=False)  # one row of 1000
    test = sp.csr_matrix((np.ones(sum(len(r) for r in per_user), np.float32), np.concatenate(per_user),
                          np.concatenate([[0], np.cumsum([len(r) for r in per_user])])), shape=(n_rows, I))
    mask, tgt = DeviceCSR(train, dev), DeviceCSR(test, dev)
    G = tgt.max_row_len
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per launch on [n, I] float32 scores of the Yelp shape, the mask picked by user id: gdmcf_rank_targets_f32 "
                    "(about 10 targets per user, one row of 1000) vs gdmcf_topk_masked_rows_f32 at k = 20 and k = 100, between HIP "
                    "events; median and max - min over rounds of alternating legs; score_gbs = 4 n I bytes over the median",
               config=dict(n_items=I, pool_rows=n_rows, G=G, long_row=args.long_row, reps=args.reps, rounds=args.rounds, warmup=args.warmup,
                           device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, kernels={}, evaluate={})
    st = _lib.stream_ptr()
    mp = (mask.indptr.data_ptr(), mask.indices.data_ptr(), None, None)
    for n in (int(s) for s in args.sizes.split(",")):
        scores = torch.randn(n, I, device=dev)
        ids = torch.arange(n, device=dev)
        ranks = torch.empty(n, G, dtype=torch.int32, device=dev)
        live = torch.empty(n, dtype=torch.int32, device=dev)
        idx = {k: torch.empty(n, k, dtype=torch.int64, device=dev) for k in (20, 100)}

        def rank_leg():
            _lib.check(lib.gdmcf_rank_targets_f32(scores.data_ptr(), scores.stride(0), n, I, *mp, tgt.indptr.data_ptr(),
                                                  tgt.indices.data_ptr(), ids.data_ptr(), G, ranks.data_ptr(), ranks.stride(0),
                                                  live.data_ptr(), st))

        def topk_leg(k):
            _lib.check(lib.gdmcf_topk_masked_rows_f32(scores.data_ptr(), scores.stride(0), n, I, *mp, ids.data_ptr(), None, k,
                                                      idx[k].data_ptr(), None, st))

        legs = {"rank": rank_leg, "topk20": lambda: topk_leg(20), "topk100": lambda: topk_leg(100)}
        ms = {name: [] for name in legs}
        for _ in range(args.rounds):
            for name, leg in legs.items():
                for _ in range(args.warmup):
                    leg()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    leg()
                e1.record()
                torch.cuda.synchronize()
                ms[name].append(e0.elapsed_time(e1) / args.reps)
        res = {}
        for name in legs:
            med = statistics.median(ms[name])
            res[f"{name}_ms"] = round(med, 5)
            res[f"{name}_legs_ms"] = [round(t, 5) for t in ms[name]]
            res[f"{name}_spread_ms"] = round(max(ms[name]) - min(ms[name]), 5)
            res[f"{name}_score_gbs"] = round(4.0 * n * I / med / 1e6, 1)
        # the two launches agree: the items of the top-20 list carry the ranks 0..19 when they are named as targets
        top = idx[20].cpu().numpy()
        rk, tip, tix = ranks.cpu().numpy(), tgt.indptr.cpu().numpy(), tgt.indices.cpu().numpy()
        ok = all(rk[b, j] == list(top[b]).index(t) for b in range(n) for j, t in enumerate(tix[tip[b]:tip[b + 1]]) if t in top[b])
        res["ranks_agree_with_top20"] = bool(ok)
        out["kernels"][f"n={n}"] = res
        print(f"n={n}", json.dumps(res), flush=True)
        del scores
    # driver.evaluate(recommend=True) with and without ranks=True
    torch.manual_seed(0)
    model, diffusion, _, _ = _pair("dnn", I, 1000, 5, U, dev)
    model = model.to(dev).eval()
    nu, topN = args.eval_users, [10, 20, 50, 100]
    tr, te = train[:nu], test[:nu]
    dtr = DeviceCSR(tr, dev)
    calls = {"lists": lambda: driver.evaluate(diffusion, model, dtr, te, dtr, topN, 0, False, 400, dev, recommend=True),
             "ranks": lambda: driver.evaluate(diffusion, model, dtr, te, dtr, topN, 0, False, 400, dev, recommend=True, ranks=True)}
    wall, got = {name: [] for name in calls}, {}
    for _ in range(args.rounds):
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = call()
            torch.cuda.synchronize()
            wall[name].append(1e3 * (time.perf_counter() - t0))
    ev = dict(users=nu, topN=topN, batch_size=400, route=diffusion.last_recommend_route, same_metrics=bool(got["lists"] == got["ranks"]))
    for name in calls:
        ev[f"{name}_wall_ms"] = round(statistics.median(wall[name]), 3)
        ev[f"{name}_wall_legs_ms"] = [round(t, 3) for t in wall[name]]
        ev[f"{name}_wall_spread_ms"] = round(max(wall[name]) - min(wall[name]), 3)
    out["evaluate"] = ev
    print("evaluate", json.dumps(ev), flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
