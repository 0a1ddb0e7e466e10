"""LightGCN trained by the fused BPR step on synthetic interactions, with the sampler's two knobs:

    python examples/train_lightgcn_synthetic.py                                   # one uniform negative per positive
    python examples/train_lightgcn_synthetic.py --n-negs 4                        # four negatives per positive
    python examples/train_lightgcn_synthetic.py --n-negs 2 --neg-pool 8           # each the best-scored of 8 candidates

The epoch loop of the reference (lightGCN.py:273-338): `BPRTrainer.train_epoch` for ceil(users / batch) steps, then
`get_metrics` on the held-out interactions.  Users interact with popularity-skewed items drawn from --seed; a fifth of every
user's interactions (at least one where the user has two) is held out.  One line per epoch:

    epoch 1 mf=0.6512 reg=0.0003 recall@20=0.0831 ndcg@20=0.0540
"""
import argparse
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gdmcf_amd  # noqa: E402
from gdmcf_amd.lightgcn import BPRTrainer, get_metrics  # noqa: E402


def synthetic_interactions(n_users, n_items, seed):
    """(train, test): scipy CSR [n_users, n_items]; 4-23 distinct items per user, item popularity ~ 1 / (rank + 10)"""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(n_items) + 10.0)
    p /= p.sum()
    tr_u, tr_i, te_u, te_i = [], [], [], []
    for u in range(n_users):
        items = rng.choice(n_items, size=min(int(rng.integers(4, 24)), n_items - 1), replace=False, p=p)
        n_test = max(1, len(items) // 5)
        te_u += [u] * n_test
        te_i += items[:n_test].tolist()
        tr_u += [u] * (len(items) - n_test)
        tr_i += items[n_test:].tolist()
    mk = lambda uu, ii: sp.csr_matrix((np.ones(len(uu), np.float32), (uu, ii)), shape=(n_users, n_items))
    return mk(tr_u, tr_i), mk(te_u, te_i)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=5000)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--n-negs", type=int, default=1, help="negatives per positive")
    ap.add_argument("--neg-pool", type=int, default=1, help="candidates per negative: the best-scored one is kept")
    ap.add_argument("--batch", type=int, default=1024, help="(user, positive) pairs per step")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--decay", type=float, default=1e-4)
    ap.add_argument("--topk", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    train, test = synthetic_interactions(args.users, args.items, args.seed)
    coo = train.tocoo()
    torch.manual_seed(args.seed)
    model = gdmcf_amd.LightGCN({"user_id_idx": coo.row, "item_id_idx": coo.col}, args.users, args.items, args.layers, args.dim,
                               device=dev).to(dev)
    batch = min(args.batch, args.users)
    trainer = BPRTrainer(model, train, batch_size=batch, lr=args.lr, decay=args.decay, seed=args.seed, n_negs=args.n_negs,
                         neg_pool=args.neg_pool)
    steps = -(-args.users // batch)
    K = min(args.topk, args.items)
    for epoch in range(1, args.epochs + 1):
        mf, reg = trainer.train_epoch(steps)
        with torch.no_grad():
            fu, fi, _, _ = model.propagate_through_layers()
        recall, _, ndcg, _ = get_metrics(fu, fi, args.users, args.items, train, test, K)
        print(f"epoch {epoch} mf={float(mf):.4f} reg={float(reg):.4f} recall@{K}={recall:.4f} ndcg@{K}={ndcg:.4f}", flush=True)
    if int(trainer.flag):
        raise RuntimeError("the sampler met a user it could not draw for")


if __name__ == "__main__":
    main()
