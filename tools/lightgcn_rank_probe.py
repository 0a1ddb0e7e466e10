"""LightGCN exact ranks, materialised vs fused, back to back in one process.

    python tools/lightgcn_rank_probe.py [--rounds 5] [--reps 3] [--targets 10] [--out-dir profiles]

For every asked user: the exact catalogue rank of `targets` held-out items by dot(user_emb[u], item_emb[i]), d = 64, the user's
training interactions masked (~25.6 per row), Xavier tables, at the Yelp shape (54 574 users, 34 395 items).  Two routes alternate
for `rounds` rounds after an untimed clock pre-heat (bench.clock_preheat) and one untimed pass of each:
  A  the route a user had before gdmcf_score_rank_f32: per chunk of 400 users torch.matmul writes the [400, I] scores into one
     reused buffer and gdmcf_rank_targets_f32 ranks the targets on the stored rows;
  B  fused: one evaluate_utils.score_rank call (gdmcf_score_rank_f32: the scores never leave the chip).
Two cases: 400 users, and all users.  A leg = `reps` full rankings between two device events (device time, warm).  Writes
<out-dir>/lightgcn_rank_probe_yelp.json: medians, every leg, max - min spreads, B's achieved TFLOP/s on the 2 U I d FLOPs of the
product against the 157.3 TFLOP/s f32 matrix peak, the bytes either route allocates beside its outputs, and how far the two
routes' ranks differ (their scores round differently: ranks of near-ties may differ by a few places; n_live must be equal).
--routes B (or A) runs one route alone, for a per-kernel profile of it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

YELP = dict(n_users=54574, n_items=34395, nnz=1_400_000)
PEAK_F32_MATRIX_TFLOPS = 157.3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--targets", type=int, default=10)
    ap.add_argument("--routes", default="A,B")
    ap.add_argument("--cases", default="400,all")
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args(argv)

    from bench import clock_preheat
    from gdmcf_amd import _lib
    from gdmcf_amd.evaluate_utils import score_rank

    dev = torch.device("cuda:0")
    lib = _lib.load()
    d, G, B = 64, args.targets, 400
    U, I, nnz = YELP["n_users"], YELP["n_items"], YELP["nnz"]
    routes = args.routes.split(",")
    rng = np.random.default_rng(0)
    xav = lambda n: torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32) * np.float32(np.sqrt(6.0 / (n + d)))).to(dev)
    ue, ie = xav(U), xav(I)
    ln = rng.poisson(nnz / U, U)
    ip_h = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    ix_h = rng.integers(0, I, int(ip_h[-1])).astype(np.int32)
    tp_h = (np.arange(U + 1) * G).astype(np.int64)
    tx_h = rng.integers(0, I, U * G).astype(np.int32)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    doc = dict(what="ms per exact ranking (the catalogue rank of every target of every asked user, training interactions masked), d = 64, "
                    "device time between events: A = per 400-user chunk torch.matmul into a [400, I] buffer + gdmcf_rank_targets_f32; "
                    "B = one fused gdmcf_score_rank_f32 call; alternating legs in one process, median over rounds",
               config=dict(shape="yelp", n_users=U, n_items=I, d=d, targets_per_row=G, chunk=B, mask_nnz=int(ip_h[-1]), rounds=args.rounds,
                           reps=args.reps, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, cases={})
    for case in args.cases.split(","):
        n = U if case == "all" else int(case)
        users = np.arange(n, dtype=np.int64) if n == U else np.sort(rng.choice(U, n, replace=False)).astype(np.int64)
        sub = lambda p, x: (np.concatenate([[0], np.cumsum(p[users + 1] - p[users])]).astype(np.int64),
                            np.concatenate([x[p[u]:p[u + 1]] for u in users] + [np.zeros(0, x.dtype)]))
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        (ip_s, ix_s), (tp_s, tx_s) = sub(ip_h, ix_h), sub(tp_h, tx_h)
        ip, ix, tp, tx, ids = to(ip_s), to(ix_s), to(tp_s), to(tx_s), to(users)
        # route A ranks chunk c's rows through the `rows` argument: the CSRs of the asked users whole, row b of the chunk = row b0 + b
        chunks = [(b0, min(b0 + B, n)) for b0 in range(0, n, B)]
        rows_all = torch.arange(n, dtype=torch.int64, device=dev)
        scores = torch.empty(B, I, dtype=torch.float32, device=dev)
        ie_t = ie.t()
        out_a = torch.empty(n, G, dtype=torch.int32, device=dev)
        live_a = torch.empty(n, dtype=torch.int32, device=dev)

        def route_a():
            st = _lib.stream_ptr()
            for b0, b1 in chunks:
                torch.matmul(ue[ids[b0:b1]], ie_t, out=scores[:b1 - b0])
                _lib.check(lib.gdmcf_rank_targets_f32(scores.data_ptr(), scores.stride(0), b1 - b0, I, ip.data_ptr(), ix.data_ptr(), None,
                                                      None, tp.data_ptr(), tx.data_ptr(), rows_all[b0:b1].data_ptr(), G,
                                                      out_a[b0:b1].data_ptr(), out_a.stride(0), live_a[b0:b1].data_ptr(), st))
            return out_a, live_a

        def route_b():
            return score_rank(ue, ie, tp, tx, ip, ix, user_ids=ids, G=G, return_live=True, check_ids=False)

        run = {"A": route_a, "B": route_b}
        res = {r: tuple(t.clone() for t in run[r]()) for r in routes}  # untimed first pass of each route (code objects, allocator)
        torch.cuda.synchronize()
        legs = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r in routes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    run[r]()
                e1.record()
                torch.cuda.synchronize()
                legs[r].append(e0.elapsed_time(e1) / args.reps)
        flops = 2.0 * n * I * d
        out = dict(n_rows=n, product_gflop=round(flops / 1e9, 2), floor_ms_at_peak=round(flops / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e3, 4),
                   score_matrix_bytes=4 * n * I, A_buffer_bytes=4 * B * I, B_workspace_bytes=int(lib.gdmcf_score_rank_ws_bytes(n, I, d, G)))
        for r in routes:
            out[f"{r}_ms"] = round(statistics.median(legs[r]), 4)
            out[f"{r}_legs_ms"] = [round(v, 4) for v in legs[r]]
            out[f"{r}_spread_ms"] = round(max(legs[r]) - min(legs[r]), 4)
        if "B" in legs:
            tf = flops / (out["B_ms"] * 1e-3) / 1e12
            out.update(B_tflops=round(tf, 2), B_frac_of_f32_matrix_peak=round(tf / PEAK_F32_MATRIX_TFLOPS, 4))
        if "A" in legs and "B" in legs:
            noise = max(out["A_spread_ms"], out["B_spread_ms"])
            diff = (res["A"][0].to(torch.int64) - res["B"][0].to(torch.int64)).abs()
            out.update(A_over_B=round(out["A_ms"] / out["B_ms"], 3), saved_ms=round(out["A_ms"] - out["B_ms"], 4), noise_ms=noise,
                       B_faster_beyond_noise=bool(out["A_ms"] - out["B_ms"] > noise),
                       ranks_compared=int(diff.numel()), ranks_that_differ=int((diff != 0).sum()), largest_rank_difference=int(diff.max()),
                       same_n_live=bool(torch.equal(res["A"][1], res["B"][1])))
        doc["cases"][case] = out
        del ip, ix, tp, tx, ids, scores, out_a, live_a, res
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "lightgcn_rank_probe_yelp.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
