"""The reverse loop (p_sample, sampling_steps = 0) in item space vs in the first hidden layer's space (`latent=True`),
back to back in one process on the same model: this probe is how the latent route is measured (bench.py times the training step).

    python tools/latent_probe.py [--iters 10] [--warmup 2] [--rounds 5] [--out profiles/latent_probe_yelp.json]
    python tools/latent_probe.py --mean-type eps --backbones dnn,onehot,dnncat [--batch 16]      (latent="extended")
    python tools/latent_probe.py --backbones dnncat                                              (DNNCat under the x0 target)

Yelp shape (34 395 items, hid 1000, batch 400, T = 5), f32, eval mode, steps = 0, dense rows, no sampling noise, the four backbones
that have the loop.  After the same untimed clock pre-heat as bench.py, each backbone alternates the two legs for `rounds` rounds;
every leg runs `warmup` untimed loops, then `iters` loops between two HIP events.  Per backbone the JSON document holds
  item_ms_per_loop / latent_ms_per_loop   median over the rounds (the item leg is the untouched default route);
  *_legs_ms, *_spread_ms                  every round; max - min of the rounds (the noise a difference has to exceed);
  operand_build_ms                        one latent loop right after a weight's version moved, minus the median loop;
  break_even_batches                      operand_build_ms / (item - latent): batches of one evaluation pass that pay the build back
                                          (null when the latent loop is not faster);
  step_kernel_us                          gdmcf_latent_step_f32 alone at the loop's shape, mean of 50 launches between two events;
  oracle_*                                deviation of both routes from the CPU oracle in float64 on the first `--oracle-rows`
                                          rows, relative to the largest |prediction| (the project's bound is 2e-5);
  topk_overlap                            mean share of the item route's top-20 items (history not masked) that the latent route's
                                          top-20 holds, on the same rows.
With --mean-type eps or the backbone dnncat the latent leg is p_sample(latent="extended") (the item leg stays the untouched
default route; dnncat has no CPU oracle class: its oracle_* fields are absent), and with --mean-type eps the document also holds
  acc_fused_us / acc_split_us             T - 1 gdmcf_latent_step_ex_f32 launches that keep the accumulator themselves, against
                                          T - 1 launches without it plus T - 1 gdmcf_latent_acc_f32 launches, alternating rounds;
                                          *_legs_us, *_spread_us as above; acc_fused_wins: the difference exceeds the larger spread."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BACKBONES = ("dnn", "onehot", "onehot-emb", "onehot-gcn")  # the default set; "dnncat" on request


def _pair(backbone, I, hid, T, U, dev, mean_type="x0"):
    import gdmcf_amd
    from oracle import gdmcf_oracle as O
    mt, omt = ((gdmcf_amd.ModelMeanType.START_X, O.ModelMeanType.START_X) if mean_type == "x0" else
               (gdmcf_amd.ModelMeanType.EPSILON, O.ModelMeanType.EPSILON))
    if backbone == "dnncat":
        model = gdmcf_amd.DNNCat([I, hid], [hid, I], 10)
        return model, gdmcf_amd.GaussianDiffusionDiscrete(mt, "linear-var", 0.01, 0.001, 0.01, T, dev, CatOneHot=True), None, None
    if backbone == "dnn":
        model = gdmcf_amd.DNN([I, hid], [hid, I], 10, time_type="cat", norm=False)
        diffusion = gdmcf_amd.GaussianDiffusion(mt, "linear-var", 0.01, 0.001, 0.01, T, dev)
        return model, diffusion, (lambda: O.DNN([I, hid], [hid, I], 10)), O.GaussianDiffusion(omt, "linear-var", 0.01, 0.001, 0.01, T)
    kw = dict(item_num=I, user_num=U)
    cls, ocls, kw = {"onehot": (gdmcf_amd.DNNOneHot, O.DNNOneHot, {}), "onehot-emb": (gdmcf_amd.DNNOneHotEmbedding, O.DNNOneHotEmbedding, kw),
                     "onehot-gcn": (gdmcf_amd.DNNOneHotEmbeddingGCN, O.DNNOneHotEmbeddingGCN, kw)}[backbone]
    model = cls([I, hid], [hid, I], 10, time_type="cat", norm=False, **kw)
    diffusion = gdmcf_amd.GaussianDiffusionDiscrete(mt, "linear-var", 0.01, 0.001, 0.01, T, dev, CatOneHot=True)
    od = O.GaussianDiffusionDiscrete(omt, "linear-var", 0.01, 0.001, 0.01, T, CatOneHot=True)
    diffusion.indexIn = od.indexIn = backbone != "onehot"
    return model, diffusion, (lambda: ocls([I, hid], [hid, I], 10, **kw)), od


def _oracle64(make, od, model, x, index):
    """The CPU oracle in float64 on the device model's weights, rows `x` (CPU float32)."""
    from oracle import gdmcf_oracle as O
    real = O.timestep_embedding
    O.timestep_embedding = lambda t, d, *a: real(t, d, *a).double()
    try:
        om = make()
        om.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
        om = om.double().eval()
        with torch.no_grad():
            kw = dict(index=index) if index is not None else {}
            return od.p_sample(om, x.double(), 0, False, **kw).numpy()
    finally:
        O.timestep_embedding = real


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--preheat-seconds", type=float, default=1.5)
    ap.add_argument("--backbones", default=",".join(BACKBONES))
    ap.add_argument("--oracle-rows", type=int, default=8, help="rows compared with the float64 oracle (0: skip)")
    ap.add_argument("--mean-type", default="x0", choices=["x0", "eps"])
    ap.add_argument("--batch", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)

    import scipy.sparse as sp

    from bench import clock_preheat
    from gdmcf_amd import _lib, data
    from gdmcf_amd import engine_core as core
    from gdmcf_amd.data_utils import DeviceCSR

    dev = torch.device("cuda:0")
    lib = _lib.load()
    B, hid, T, n_pool, k = args.batch, 1000, 5, 4, 20
    indptr, indices, I = data.synth_csr("yelp", n_rows=n_pool * B, seed=0)
    U = data.SHAPES["yelp"]["n_users"]
    dcsr = DeviceCSR(sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n_pool * B, I)), dev)
    row_ids = [torch.arange(i * B, (i + 1) * B, device=dev) for i in range(n_pool)]
    x_buf = torch.empty(B, I, dtype=torch.float32, device=dev)
    preheat = clock_preheat(lib, dev, args.preheat_seconds)
    out = dict(what="ms per reverse loop (p_sample, steps = 0, T = 5, dense rows, no sampling noise), item space vs the first hidden "
                    "layer's space (latent=True; latent=\"extended\" for the eps target and dnncat), Yelp shape, f32, eval mode; HIP "
                    "events, median over rounds of alternating legs",
               config=dict(mean_type=args.mean_type, n_items=I, n_users=U, hidden=hid, batch=B, T=T, iters=args.iters, warmup=args.warmup, rounds=args.rounds,
                           oracle_rows=args.oracle_rows, device=torch.cuda.get_device_name(dev)),
               clock_preheat=preheat, backbones={})

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    for backbone in args.backbones.split(","):
        torch.manual_seed(0)
        model, diffusion, make_oracle, od = _pair(backbone, I, hid, T, U, dev, args.mean_type)
        spelling = "extended" if (args.mean_type == "eps" or backbone == "dnncat") else True
        model = model.to(dev).eval()
        with_index = backbone in ("onehot-emb", "onehot-gcn")
        kw = [dict(index=r) if with_index else {} for r in row_ids]
        pred = {}

        def loop(leg, i):
            pred[leg] = diffusion.p_sample(model, dcsr.rows(row_ids[i % n_pool], out=x_buf), 0, False,
                                           latent=spelling if leg == "latent" else False, **kw[i % n_pool])
            assert diffusion.last_reverse_route == leg

        legs = {"item": [], "latent": []}
        for _ in range(args.rounds):
            for leg in legs:
                for i in range(args.warmup):  # (the first warm-up loop also builds the cached operands of the weights)
                    loop(leg, i)
                torch.cuda.synchronize()
                legs[leg].append(timed(lambda i: loop(leg, i), args.iters))
        res = {}
        for leg, v in legs.items():
            res[f"{leg}_ms_per_loop"] = round(statistics.median(v), 4)
            res[f"{leg}_legs_ms"] = [round(t, 4) for t in v]
            res[f"{leg}_spread_ms"] = round(max(v) - min(v), 4)
        d, c = res["item_ms_per_loop"], res["latent_ms_per_loop"]
        res.update(saved_ms=round(d - c, 4), saved_frac=round((d - c) / d, 4),
                   exceeds_spread=bool(d - c > max(res["item_spread_ms"], res["latent_spread_ms"])))
        # the one-off operand build: a loop right after a weight's version moved
        builds = []
        for _ in range(3):
            torch.autograd.graph.increment_version(model.in_layers[0].weight)
            torch.cuda.synchronize()
            builds.append(timed(lambda i: loop("latent", i), 1) - c)
        res["operand_build_ms"] = round(statistics.median(builds), 4)
        res["break_even_batches"] = round(res["operand_build_ms"] / (d - c), 2) if d > c else None
        # the step kernel alone at the loop's shape
        ops = model.engine._latent[1]
        Kl = {"dnn": hid, "dnncat": hid, "onehot": 2 * hid}.get(backbone, 3 * hid)  # [h], [h | h_U], [h | h_U | user row]
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.tanh(torch.randn(B, ops.M.stride(0), generator=g, device=dev))
        p = torch.randn(B, 1024, generator=g, device=dev)
        h = torch.empty_like(p)
        c1 = torch.full((B,), 0.5, device=dev)
        st = _lib.stream_ptr()
        step = lambda i: core.latent_step(lib, A, ops.M, ops.v, p, c1, c1, ops.e[0], 1, B, hid, Kl, p, h, st)
        timed(step, 5)
        res["step_kernel_us"] = round(1e3 * timed(step, 50), 3)
        res["step_kernel_shape"] = [B, hid, Kl]
        if args.mean_type == "eps":
            # the accumulator inside the step kernel against launches of its own: T - 1 steps of a loop each way
            Q = torch.zeros(B, ops.M.stride(0), device=dev)
            acc = (Q, c1, c1, Q)

            def fused(i):
                for _ in range(T - 1):
                    core.latent_step_ex(lib, A, ops.M, ops.v, p, c1, c1, None, ops.e[0], 1, B, hid, Kl, p, h, acc, st)

            def split(i):
                for _ in range(T - 1):
                    core.latent_step_ex(lib, A, ops.M, ops.v, p, c1, c1, None, ops.e[0], 1, B, hid, Kl, p, h, None, st)
                    core.latent_acc(lib, Q, c1, A, c1, B, Kl, Q, st)

            ways = {"acc_fused": [], "acc_split": []}
            for _ in range(args.rounds):
                for name, fn in (("acc_fused", fused), ("acc_split", split)):
                    timed(fn, 5)
                    ways[name].append(1e3 * timed(fn, 50))
            for name, v in ways.items():
                res[f"{name}_us"] = round(statistics.median(v), 3)
                res[f"{name}_legs_us"] = [round(t, 3) for t in v]
                res[f"{name}_spread_us"] = round(max(v) - min(v), 3)
            res["acc_fused_wins"] = bool(res["acc_split_us"] - res["acc_fused_us"] > max(res["acc_fused_spread_us"], res["acc_split_spread_us"]))
        # both routes against the float64 oracle, and the top-k sets, on a sample of rows
        loop("item", 0)
        loop("latent", 0)
        torch.cuda.synchronize()
        n = args.oracle_rows
        ti, tl = pred["item"].topk(k, dim=1).indices.cpu().numpy(), pred["latent"].topk(k, dim=1).indices.cpu().numpy()
        res["topk_overlap"] = round(float(np.mean([len(set(a) & set(b)) / k for a, b in zip(ti, tl)])), 6)
        res["max_abs_item_minus_latent"] = float((pred["item"] - pred["latent"]).abs().max())
        res["max_abs_pred"] = float(pred["item"].abs().max())
        if n > 0 and make_oracle is not None:
            ref = _oracle64(make_oracle, od, model, dcsr.rows(row_ids[0][:n]).cpu(), row_ids[0][:n].cpu() if with_index else None)
            scale = float(np.abs(ref).max())
            for leg in legs:
                res[f"oracle_dev_{leg}"] = float(np.abs(pred[leg][:n].cpu().double().numpy() - ref).max() / max(scale, 1e-30))
            tr = np.argsort(-ref, axis=1)[:, :k]
            res["oracle_topk_overlap_latent"] = round(float(np.mean([len(set(a) & set(b)) / k for a, b in zip(tr, tl[:n])])), 6)
            res["oracle_topk_overlap_item"] = round(float(np.mean([len(set(a) & set(b)) / k for a, b in zip(tr, ti[:n])])), 6)
        out["backbones"][backbone] = res
        print(backbone, json.dumps(res), flush=True)
        del model, diffusion, ops, pred
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
