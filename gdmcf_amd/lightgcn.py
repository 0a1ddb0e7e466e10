"""LightGCN embedding propagation with the reference's interface (reference lightGCN.py:129-203).

`get_A_tilda` builds the symmetric-normalised bipartite adjacency D^-1/2 A D^-1/2 once on the host (float32, as the
reference), keeps it on the GPU as CSR and builds the SpMM's static schedule (spmm_schedule.SpmmSchedule) for the kernel
generation pick_generation chooses: streamed (gdmcf_spmm_stream_f32) while an eighth of the table fits one XCD's L2, the
first-generation virtual rows (gdmcf_spmm_csr_f32) above that and at other widths; GDMCF_SPMM_GEN forces one, the bundled
second generation included.  `propagate_through_layers` runs one `SpmmSchedule.launch` per layer, the layer mean fused into
the last one's epilogue; the propagation serves as its own backward: A~ is symmetric (`_PropagateMean`).
Re-exported under their old names: the schedule builders and GDMCF_SPMM_* knobs (spmm_schedule.py), the ranking metrics
(lightgcn_eval.py), BPR training (bpr.py).
"""
import os

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from . import _lib
from .bpr import (BPRTrainer, _bpr_grad, _bpr_loss, _bpr_operands, _bpr_order, _bpr_sample, _bpr_sample_pool, bpr_loss,  # noqa: F401
                  bpr_loss_grad, bpr_reg_grad_, sample_bpr_batch, sample_bpr_items, sample_bpr_negatives)
from .lightgcn_eval import _check_Ks, _history_rows, get_metrics, get_metrics_at, hits_from_ranks, ranking_terms  # noqa: F401
from .spmm_schedule import (SPMM_CHUNK, SPMM_COST_PIECE, SPMM_COST_ROW, SPMM_HOT_MB, SPMM_MISS_W, SPMM_NT, SPMM_PIECE,  # noqa: F401
                            SPMM_SHORT, SPMM_SLICE_MB, SPMM_SMAX, SPMM_WAVES, SpmmSchedule, pick_generation, spmm_bundle_plan,
                            spmm_plan, spmm_stream_pack)


def normalized_bipartite_csr(users, items, n_users, n_items):
    """CSR (indptr int64, indices int32, data float32) of A~ = D^-1/2 [[0,R],[R^T,0]] D^-1/2,
    d = (rowsum + 1e-9)^-1/2 in float32, duplicates collapsed (reference :146-164)."""
    users = np.asarray(users, dtype=np.int64)
    items = np.asarray(items, dtype=np.int64)
    R = sp.coo_matrix((np.ones(len(users), np.float32), (users, items)), shape=(n_users, n_items)).tocsr()
    R.data[:] = 1.0
    A = sp.bmat([[None, R], [R.T.tocsr(), None]], format="csr", dtype=np.float32)
    A.sort_indices()
    N = n_users + n_items
    rowsum = np.asarray(A.sum(1), dtype=np.float32).flatten()
    d = np.power(rowsum + np.float32(1e-9), np.float32(-0.5)).astype(np.float32)
    d[np.isinf(d)] = 0.0
    rows = np.repeat(np.arange(N), np.diff(A.indptr))
    data = ((d[rows] * A.data).astype(np.float32) * d[A.indices]).astype(np.float32)
    return A.indptr.astype(np.int64), A.indices.astype(np.int32), data



class LightGCN(nn.Module):
    def __init__(self, data, n_users, n_items, n_layers, latent_dim, device="cuda", shard_rows=False, group=None):
        """data: DataFrame/dict with `user_id_idx` / `item_id_idx` columns (reference :147).

        shard_rows (new, multi-GPU; the reference is single-device): every rank of `group` keeps only a contiguous
        block of ceil(N/world) rows of the normalised adjacency.  A layer is then a local SpMM on the full embedding
        table of the previous layer plus an all-gather of the row blocks (N*d*4/world bytes per rank per layer over
        xGMI); the backward pass all-reduces the cotangent first -- propagation is linear, so sum_r A~^l g_r =
        A~^l sum_r g_r -- which makes E0.grad the SUM over ranks already (do not all-reduce it again)."""
        super().__init__()
        import torch.distributed as dist
        self._group = group
        self._world = dist.get_world_size(group) if (shard_rows and dist.is_initialized()) else 1
        self._rank = dist.get_rank(group) if self._world > 1 else 0
        self.data = data
        self.n_users, self.n_items = n_users, n_items
        self.n_layers, self.latent_dim = n_layers, latent_dim
        self._device = torch.device(device)
        self.init_embedding()
        self.norm_adj_csr = self.get_A_tilda()

    def init_embedding(self):
        self.E0 = nn.Embedding(self.n_users + self.n_items, self.latent_dim)
        nn.init.xavier_uniform_(self.E0.weight)
        self.E0.weight = nn.Parameter(self.E0.weight)

    def get_A_tilda(self):
        indptr, indices, vals = normalized_bipartite_csr(np.asarray(self.data["user_id_idx"]),
                                                         np.asarray(self.data["item_id_idx"]), self.n_users,
                                                         self.n_items)
        N = self.n_users + self.n_items
        rpr = -(-N // self._world)  # rows per rank
        r0 = min(self._rank * rpr, N)
        r1 = min(r0 + rpr, N)
        self._rows = (r0, r1, rpr)
        if self._world > 1:
            lo, hi = int(indptr[r0]), int(indptr[r1])
            indptr, indices, vals = indptr[r0:r1 + 1] - indptr[r0], indices[lo:hi], vals[lo:hi]
        gen = pick_generation(N, self.latent_dim, indices.size, os.environ.get("GDMCF_SPMM_GEN", "auto"))
        split = self.n_users if (os.environ.get("GDMCF_SPMM_SPLIT", "0") == "1" and self._world == 1) else None
        self._sched = SpmmSchedule(indptr, indices, vals, N, self.latent_dim, gen, split, self._device)
        self.nnz = int(indices.size)
        return (torch.from_numpy(indptr).to(self._device), self._sched.col, self._sched.val)

    # what others read of the schedule: the plan's device tensors, the partial-sum workspace, which generation it is
    _plan = property(lambda self: self._sched.plan)
    _partial = property(lambda self: self._sched.partial)
    _bundled = property(lambda self: self._sched.generation == "2")
    _streamed = property(lambda self: self._sched.generation == "3")

    def algorithmic_bytes(self):
        """Compulsory HBM bytes of one layer: CSR once, X once, Y once."""
        N, d = self.n_users + self.n_items, self.latent_dim
        rows = self._rows[1] - self._rows[0]  # this rank's block: CSR once, X once, its rows of Y once
        return self.nnz * 8.0 + (rows + 1) * 8.0 + (N + rows) * d * 4.0

    @torch.no_grad()
    def _propagate(self, X, return_layers=False):
        """mean_l (A~^l X), l = 0..n_layers: one SpMM per layer (layer mean fused into the last SpMM)."""
        _lib.require_gpu(X, "LightGCN embeddings")
        N, d = X.shape
        st = _lib.stream_ptr()
        cur = X.contiguous()
        layers = [cur]
        r0, r1, rpr = self._rows
        sharded = self._world > 1
        alg_bytes = self.algorithmic_bytes()
        for layer in range(self.n_layers):
            last = (layer == self.n_layers - 1) and not return_layers
            out = torch.zeros(rpr, d, dtype=cur.dtype, device=cur.device) if sharded else torch.empty_like(cur)
            # the fused layer mean reads this rank's rows of the earlier layers
            adds = ([a[r0:] for a in layers] if r0 else layers) if last else []
            if r1 > r0:
                self._sched.launch(cur, r1 - r0, N, out, adds, 1.0 / (self.n_layers + 1) if last else 1.0, alg_bytes, st)
            if sharded:
                from .parallel import all_gather_rows
                out = all_gather_rows(out, N, self._group)
            layers.append(out)
            cur = out
        if return_layers:
            mean = torch.stack(layers).sum(0) / (self.n_layers + 1)  # test/debug path only
            return mean, layers[1:]
        return (cur if self.n_layers > 0 else X), None

    def propagate_through_layers(self, return_layers=False):
        """(final_user, final_item, initial_user, initial_item) as reference lightGCN.py:180-194.  Differentiable
        w.r.t. E0 when autograd is on (the backward is the same propagation: A~ is symmetric)."""
        E0 = self.E0.weight
        if return_layers:
            mean, layers = self._propagate(E0.detach(), return_layers=True)
        elif torch.is_grad_enabled() and E0.requires_grad:
            mean, layers = _PropagateMean.apply(self, E0), None
        else:
            mean, layers = self._propagate(E0.detach())[0], None
        final_user, final_item = torch.split(mean, [self.n_users, self.n_items])
        init_user, init_item = torch.split(E0 if layers is None else E0.detach(), [self.n_users, self.n_items])
        if return_layers:
            return final_user, final_item, init_user, init_item, layers
        return final_user, final_item, init_user, init_item

    def forward(self, users, pos_items, neg_items):
        fu, fi, iu, ii = self.propagate_through_layers()
        return fu[users], fi[pos_items], fi[neg_items], iu[users], ii[pos_items], ii[neg_items]
    def _asked_ids(self, users, what):
        """`users` (int64 ids, any device / array) as an int64 host tensor, range-checked (on the host: no device sync)."""
        ids = torch.as_tensor(np.asarray(users.cpu() if torch.is_tensor(users) else users), dtype=torch.int64)
        if ids.numel() and not (0 <= int(ids.min()) and int(ids.max()) < self.n_users):
            raise IndexError(f"{what}: user ids out of range")
        return ids

    @torch.no_grad()
    def recommend(self, users, k, history=None):
        """The k best items of `users` (int64 ids, any device / array) by the propagated embeddings, best first: int64
        [len(users), k] on the GPU.  `history` (scipy CSR or data_utils.DeviceCSR, one row per user of the MODEL): the
        interactions of the asked users are excluded, as the reference's get_metrics excludes the training set
        (lightGCN.py:77-86).  One propagation + evaluate_utils.score_topk: no [users, items] score matrix."""
        from .evaluate_utils import score_topk
        fu, fi, _, _ = self.propagate_through_layers()
        ids = self._asked_ids(users, "recommend").to(fu.device)
        ip, ix = _history_rows(history, ids)
        return score_topk(fu, fi, k, ip, ix, user_ids=ids, check_ids=False)

    @torch.no_grad()
    def rank_targets(self, users, targets, history=None, return_live=False):
        """The exact catalogue rank of every target item of `users` (int64 ids, any device / array) by the propagated
        embeddings: int32 [len(users), G] on the GPU, G = the longest target row of the asked users (at least 1; one host read),
        ranks[b, j] = the place target j of user users[b] has in recommend(users, k = n_items, history)'s list, -1 past the
        row's length.  `targets` and `history` (optional): scipy CSR or data_utils.DeviceCSR with one row per user of the MODEL;
        the history of the asked users counts as -inf, as in recommend.  With `return_live` also the number of unmasked items
        per user (int32 [len(users)]).  One propagation + evaluate_utils.score_rank: no [users, items] score matrix, no k."""
        from .evaluate_utils import score_rank
        if targets is None:
            raise ValueError("rank_targets: targets (scipy CSR or DeviceCSR, one row per user) are required")
        for m, what in ((targets, "targets"), (history, "history")):
            if m is not None and tuple(m.shape) != (self.n_users, self.n_items):
                raise ValueError(f"rank_targets: {what} has shape {tuple(m.shape)}, the model has {(self.n_users, self.n_items)}")
        ids = self._asked_ids(users, "rank_targets")
        fu, fi, _, _ = self.propagate_through_layers()
        ids = ids.to(fu.device)
        ip, ix = _history_rows(history, ids)
        tp, tx = _history_rows(targets, ids)
        return score_rank(fu, fi, tp, tx, ip, ix, user_ids=ids, return_live=return_live, check_ids=False)


class _PropagateMean(torch.autograd.Function):
    """mean over layers of A~^l E0.  d(mean)/d(E0) applied to a cotangent G is mean_l (A~^l)^T G = mean_l A~^l G
    because the normalised adjacency is symmetric (reference lightGCN.py:149-164): the backward pass is the
    forward kernel run on the gradient."""

    @staticmethod
    def forward(ctx, module, E0):
        ctx.module = module
        return module._propagate(E0.detach())[0]

    @staticmethod
    def backward(ctx, g):
        m = ctx.module
        g = g.contiguous()
        if m._world > 1:  # row-sharded: propagate the SUM of all ranks' cotangents (linearity), see LightGCN.__init__
            from .parallel import _all_reduce
            g = g.clone()
            _all_reduce(g, m._group)
        return None, m._propagate(g)[0]

