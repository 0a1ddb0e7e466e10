"""LightGCN ranking, unfused vs fused, back to back in one process.

    python tools/lightgcn_eval_probe.py [--shapes yelp,amazon] [--rounds 5] [--reps 3] [--out-dir profiles]

For every user: the k = 100 best items by dot(user_emb[u], item_emb[i]), d = 64, the user's training interactions excluded
(reference lightGCN.py:67-127, get_metrics), Xavier tables and a mask of the data set's density.  Two routes alternate for
`rounds` rounds after an untimed clock pre-heat (bench.clock_preheat) and one untimed pass of each:
  A  unfused, what the library could do before gdmcf_score_topk_f32: per block of 400 users gdmcf_linear_fwd_f32 writes the
     [400, I] scores, masked_topk (gdmcf_topk_masked_f32) reads them back;
  B  fused: one evaluate_utils.score_topk call over all users (gdmcf_score_topk_f32: the scores never leave the chip).
A leg = `reps` full rankings, timed with a host clock around a device synchronise.  Writes one JSON document per shape to
<out-dir>/lightgcn_eval_probe_<shape>.json: medians, every leg, max - min spreads, B's achieved TFLOP/s on the 2 U I d FLOPs of
the product against the 157.3 TFLOP/s f32 matrix peak, and whether both routes returned the same lists.  --routes B (or A)
runs one route alone, for a per-kernel profile of it."""
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

SHAPES = {"yelp": dict(n_users=54574, n_items=34395, nnz=1_400_000), "amazon": dict(n_users=108822, n_items=94949, nnz=3_150_000)}
PEAK_F32_MATRIX_TFLOPS = 157.3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="yelp,amazon")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--routes", default="A,B")
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args(argv)

    from bench import clock_preheat
    from gdmcf_amd import _lib
    from gdmcf_amd.evaluate_utils import masked_topk, score_topk

    dev = torch.device("cuda:0")
    lib = _lib.load()
    d, k, B = 64, 100, 400
    routes = args.routes.split(",")
    for shape in args.shapes.split(","):
        U, I, nnz = (SHAPES[shape][n] for n in ("n_users", "n_items", "nnz"))
        rng = np.random.default_rng(0)
        xav = lambda n: torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32) * np.float32(np.sqrt(6.0 / (n + d)))).to(dev)
        ue, ie = xav(U), xav(I)
        ln = rng.poisson(nnz / U, U)
        ip_h = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        ip = torch.from_numpy(ip_h).to(dev)
        ix = torch.from_numpy(rng.integers(0, I, int(ip_h[-1])).astype(np.int32)).to(dev)
        # route A's per-block mask pointers (indptr rebased to the block: gdmcf_topk_masked_f32 takes the indices pointer as is)
        blocks = [(b0, min(b0 + B, U)) for b0 in range(0, U, B)]
        ip_blocks = [(ip[b0:b1 + 1] - ip[b0]).contiguous() for b0, b1 in blocks]
        ix_blocks = [ix[int(ip_h[b0]):int(ip_h[b1])] for b0, b1 in blocks]
        scores = torch.empty(B, I, dtype=torch.float32, device=dev)
        ws_bytes = max(int(lib.gdmcf_linear_ws_bytes(B, I, d)), 256)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out_a = torch.empty(U, k, dtype=torch.int64, device=dev)

        def route_a():
            st = _lib.stream_ptr()
            for (b0, b1), ipb, ixb in zip(blocks, ip_blocks, ix_blocks):
                _lib.check(lib.gdmcf_linear_fwd_f32(ue[b0:b1].data_ptr(), ue.stride(0), ie.data_ptr(), ie.stride(0), None, 0, b1 - b0,
                                                    I, d, scores.data_ptr(), scores.stride(0), ws.data_ptr(), ws_bytes, st))
                out_a[b0:b1] = masked_topk(scores[:b1 - b0], k, ipb, ixb)
            return out_a

        def route_b():
            return score_topk(ue, ie, k, ip, ix)

        run = {"A": route_a, "B": route_b}
        preheat = clock_preheat(lib, dev, args.preheat_seconds)
        res = {r: run[r]().clone() for r in routes}  # untimed first pass of each route (code objects, allocator)
        torch.cuda.synchronize()
        legs = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r in routes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    run[r]()
                torch.cuda.synchronize()
                legs[r].append(1e3 * (time.perf_counter() - t0) / args.reps)
        flops = 2.0 * U * I * d
        out = dict(what="ms per full ranking (top-100 of every user over all items, training interactions masked), d = 64: A = per "
                        "400-user block gdmcf_linear_fwd_f32 into a [400, I] buffer + gdmcf_topk_masked_f32; B = one fused "
                        "gdmcf_score_topk_f32 call; alternating legs in one process, median over rounds",
                   config=dict(shape=shape, n_users=U, n_items=I, d=d, k=k, block=B, mask_nnz=int(ip_h[-1]), rounds=args.rounds,
                               reps=args.reps, device=torch.cuda.get_device_name(dev)),
                   clock_preheat=preheat, product_gflop=round(flops / 1e9, 1),
                   floor_ms_at_peak=round(flops / (PEAK_F32_MATRIX_TFLOPS * 1e12) * 1e3, 4),
                   score_matrix_bytes=4 * U * I, B_workspace_bytes=int(lib.gdmcf_score_topk_ws_bytes(U, I, d, k)))
        for r in routes:
            med = statistics.median(legs[r])
            out[f"{r}_ms"] = round(med, 4)
            out[f"{r}_legs_ms"] = [round(v, 4) for v in legs[r]]
            out[f"{r}_spread_ms"] = round(max(legs[r]) - min(legs[r]), 4)
        if "B" in legs:
            tf = flops / (out["B_ms"] * 1e-3) / 1e12
            out.update(B_tflops=round(tf, 2), B_frac_of_f32_matrix_peak=round(tf / PEAK_F32_MATRIX_TFLOPS, 4))
        if "A" in legs and "B" in legs:
            noise = max(out["A_spread_ms"], out["B_spread_ms"])
            out.update(saved_ms=round(out["A_ms"] - out["B_ms"], 4), noise_ms=noise,
                       B_faster_beyond_noise=bool(out["A_ms"] - out["B_ms"] > noise),
                       same_lists=bool(torch.equal(res["A"], res["B"])),
                       rows_with_different_lists=int((res["A"] != res["B"]).any(1).sum()))
        text = json.dumps(out, indent=1)
        print(text, flush=True)
        os.makedirs(args.out_dir, exist_ok=True)
        with open(os.path.join(args.out_dir, f"lightgcn_eval_probe_{shape}.json"), "w") as f:
            f.write(text + "\n")
        del ue, ie, ip, ix, scores, ws, out_a, res
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
