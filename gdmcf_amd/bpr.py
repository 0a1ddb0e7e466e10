"""BPR training of LightGCN (reference lightGCN.py:207-251, :287-300), two routes.

`bpr_loss` + `sample_bpr_batch` around `LightGCN.forward` are the reference's script as it stands: autograd around the HIP
propagation, a host sampler.  `BPRTrainer` is the fused step (csrc/bpr.hip): triples drawn on the device
(gdmcf_bpr_sample_f32), loss and per-triple derivative in one kernel (gdmcf_bpr_loss_f32), the cotangent scattered without
atomics (gdmcf_bpr_grad_f32), the same propagation run on it, FusedAdamW -- no autograd graph, no host synchronisation.
`sample_bpr_items`, `bpr_loss_grad` and `bpr_reg_grad_` are its functional pieces; `sample_bpr_negatives`
(gdmcf_bpr_sample_pool_f32) draws several negatives per positive, each the best-scored of a pool of candidates, for the
trainer's `n_negs` / `neg_pool` knobs.
"""
import numpy as np
import torch

from . import _lib


def bpr_loss(users, users_emb, pos_emb, neg_emb, userEmb0, posEmb0, negEmb0):
    """(mf_loss, reg_loss) of reference lightGCN.py:207-219."""
    reg_loss = (1 / 2) * (userEmb0.norm().pow(2) + posEmb0.norm().pow(2) + negEmb0.norm().pow(2)) / float(len(users))
    pos_scores = torch.sum(torch.mul(users_emb, pos_emb), dim=1)
    neg_scores = torch.sum(torch.mul(users_emb, neg_emb), dim=1)
    loss = torch.mean(torch.nn.functional.softplus(neg_scores - pos_scores))
    return loss, reg_loss


def sample_bpr_batch(indptr, indices, n_users, n_items, batch_size, rng):
    """(users, pos_items, neg_items) as the reference sampler (lightGCN.py:221-251, minus its stray
    pdb.set_trace): sorted users drawn without replacement (with replacement if n_users < batch_size), one random
    interacted item and one random non-interacted item per user.  Vectorised numpy; `rng` = np.random.Generator."""
    if n_users < batch_size:
        users = np.sort(rng.integers(0, n_users, batch_size))
    else:
        users = np.sort(rng.choice(n_users, batch_size, replace=False))
    deg = indptr[users + 1] - indptr[users]
    if np.any(deg == 0):
        raise ValueError("sample_bpr_batch: every sampled user needs at least one interaction")
    pos = indices[indptr[users] + (rng.random(batch_size) * deg).astype(np.int64)]
    neg = rng.integers(0, n_items, batch_size)
    for _ in range(64):  # rejection: resample the (few) negatives that hit an interacted item
        bad = np.array([n in indices[indptr[u]:indptr[u + 1]] for u, n in zip(users, neg)]) if batch_size <= 4096 else \
            np.zeros(batch_size, bool)
        if not bad.any():
            break
        neg[bad] = rng.integers(0, n_items, int(bad.sum()))
    return users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# fused BPR step (csrc/bpr.hip): one call helper per C entry point, the functional pieces, the trainer
# ------------------------------------------------------------------------------------------------------------------
def _bpr_sample(lib, indptr, indices, users, n_users, n_items, seed, offset, pos, neg, flag, st):
    _lib.check(lib.gdmcf_bpr_sample_f32(indptr.data_ptr(), indices.data_ptr(), users.data_ptr(), users.numel(), n_users, n_items,
                                        int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), pos.data_ptr(), neg.data_ptr(),
                                        _lib.ptr(flag), st))


def _bpr_sample_pool(lib, indptr, indices, users, n_negs, pool, n_users, n_items, M, seed, offset, pos, neg, flag, st):
    """pos [B], neg [B * n_negs] (slot k of triple j at j * n_negs + k); M: the propagated table, read only when pool > 1"""
    scored = pool > 1
    _lib.check(lib.gdmcf_bpr_sample_pool_f32(indptr.data_ptr(), indices.data_ptr(), users.data_ptr(), users.numel(), n_negs, pool,
                                             n_users, n_items, M.data_ptr() if scored else None, M.stride(0) if scored else 0,
                                             M.shape[1] if scored else 0, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1),
                                             pos.data_ptr(), neg.data_ptr(), _lib.ptr(flag), st))


def _bpr_loss(lib, M, E0, users, pos, neg, n_users, n_items, coef, ws, out2, flag, st):
    """out2 float32 [2] <- (mf, reg); coef [B] <- sigmoid(x_j) / B"""
    _lib.check(lib.gdmcf_bpr_loss_f32(M.data_ptr(), M.stride(0), E0.data_ptr(), E0.stride(0), E0.shape[1], users.data_ptr(),
                                      pos.data_ptr(), neg.data_ptr(), users.numel(), n_users, n_items, coef.data_ptr(),
                                      ws.data_ptr(), out2.data_ptr(), out2.data_ptr() + 4, _lib.ptr(flag), st))


def _bpr_grad(lib, mode, order, users, pos, neg, n_users, n_items, coef, src, out, scale, zero_rows, st):
    _lib.check(lib.gdmcf_bpr_grad_f32(mode, order.data_ptr(), users.data_ptr(), pos.data_ptr(), neg.data_ptr(), users.numel(),
                                      n_users, n_items, _lib.ptr(coef), src.data_ptr(), src.stride(0), src.shape[1],
                                      out.data_ptr(), out.stride(0), float(scale), _lib.ptr(zero_rows),
                                      0 if zero_rows is None else zero_rows.stride(0), st))


def _bpr_order(users, pos, neg, n_users):
    """int32 [3B]: the batch's entries e = role * B + j (role 0 user, 1 pos, 2 neg) sorted stably by node"""
    nodes = torch.cat([users, pos + n_users, neg + n_users])
    return torch.sort(nodes, stable=True).indices.to(torch.int32)


def _bpr_operands(M, E0, users, pos, neg, n_users):
    for t, what in ((E0, "E0"), (M, "the propagated embeddings"), (users, "users"), (pos, "pos items"), (neg, "neg items")):
        if t is not None:
            _lib.require_gpu(t, f"BPR: {what}")
    for t in (E0, M):
        if t is not None and (t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.shape != E0.shape):
            raise ValueError("BPR: E0 and the propagated table must be float32 [n_users + n_items, d] with unit column stride")
    if not 0 < n_users < E0.shape[0]:
        raise ValueError("BPR: n_users must lie inside the table")
    ids = [t.to(dtype=torch.int64).contiguous() for t in (users, pos, neg)]
    if ids[0].dim() != 1 or ids[0].numel() == 0 or any(t.shape != ids[0].shape for t in ids):
        raise ValueError("BPR: users, pos and neg must be three non-empty 1-D id arrays of one length")
    return ids


@torch.no_grad()
def sample_bpr_items(indptr, indices, users, n_items, seed, offset):
    """(pos, neg, flag) for the given users by gdmcf_bpr_sample_f32 (include/gdmcf_hip.h): device CSR of the training
    interactions (indptr int64, indices int32, rows sorted and free of duplicates), users int64 on the device.  pos[j] is uniform
    over users[j]'s row, neg[j] uniform over the items outside it (exactly: the r-th missing item by binary search, no rejection
    loop); Philox counter (j, 0, 7, offset), key seed.  flag: int32 [1], 1 if a user had no positive or no negative to draw
    (pos = neg = -1 there)."""
    lib = _lib.load()
    for t, what in ((indptr, "CSR indptr"), (indices, "CSR indices"), (users, "users")):
        _lib.require_gpu(t, f"sample_bpr_items: {what}")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or users.dtype != torch.int64:
        raise ValueError("sample_bpr_items: indptr int64, indices int32, users int64 expected")
    users = users.contiguous()
    pos, neg = torch.empty_like(users), torch.empty_like(users)
    flag = torch.zeros(1, dtype=torch.int32, device=users.device)
    _bpr_sample(lib, indptr.contiguous(), indices.contiguous(), users, indptr.numel() - 1, int(n_items), seed, offset, pos, neg,
                flag, _lib.stream_ptr())
    return pos, neg, flag


@torch.no_grad()
def sample_bpr_negatives(indptr, indices, users, n_items, seed, offset, n_negs=1, pool=1, M=None):
    """(pos [B], neg [B, n_negs], flag) for the given users by gdmcf_bpr_sample_pool_f32 (include/gdmcf_hip.h): operands as
    `sample_bpr_items`.  pos[j] is that function's positive.  neg[j, k] is the best of `pool` candidates drawn uniformly (and
    independently: repeats are possible) from the items outside users[j]'s row, by the float32 score <M[users[j]], M[n_users +
    i]> -- the earliest drawn among equals; M: the propagated table, float32 [n_users + n_items, d] on the device, needed (and
    read) only when pool > 1.  n_negs = pool = 1 gives `sample_bpr_items`'s pos and neg bit for bit.  Candidate q = k * pool + c
    of triple j takes word y, z, w of the Philox block with counter (j, 0, 7, offset) for q < 3 and word (q - 3) % 4 of block
    (j, 1 + (q - 3) / 4, 7, offset) after that."""
    lib = _lib.load()
    for t, what in ((indptr, "CSR indptr"), (indices, "CSR indices"), (users, "users")):
        _lib.require_gpu(t, f"sample_bpr_negatives: {what}")
    if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or users.dtype != torch.int64:
        raise ValueError("sample_bpr_negatives: indptr int64, indices int32, users int64 expected")
    n_negs, pool, n_users = int(n_negs), int(pool), indptr.numel() - 1
    if n_negs < 1 or pool < 1:
        raise ValueError("sample_bpr_negatives: n_negs >= 1 and pool >= 1 expected")
    if pool > 1:
        if M is None:
            raise ValueError("sample_bpr_negatives: pool > 1 scores the candidates and needs the propagated table M")
        _lib.require_gpu(M, "sample_bpr_negatives: the propagated embeddings")
        if M.dim() != 2 or M.dtype != torch.float32 or M.stride(1) != 1 or M.shape[0] != n_users + int(n_items):
            raise ValueError("sample_bpr_negatives: M must be float32 [n_users + n_items, d] with unit column stride")
    users = users.contiguous()
    pos = torch.empty_like(users)
    neg = torch.empty(users.numel(), n_negs, dtype=torch.int64, device=users.device)
    flag = torch.zeros(1, dtype=torch.int32, device=users.device)
    _bpr_sample_pool(lib, indptr.contiguous(), indices.contiguous(), users, n_negs, pool, n_users, int(n_items), M, seed, offset,
                     pos, neg, flag, _lib.stream_ptr())
    return pos, neg, flag


@torch.no_grad()
def bpr_loss_grad(M, E0, users, pos, neg, n_users, decay, return_coef=False):
    """(mf, reg, G) of one batch without autograd.  M: the propagated mean table (`model._propagate(E0)[0]`), E0: the parameter,
    both [n_users + n_items, d] on the GPU; users / pos / neg: int64 device ids (pos / neg are item ids).  mf, reg: 0-d float32
    device tensors, the values of `bpr_loss`; G [N, d]: the cotangent of M under mf + decay * reg -- a fresh table, zero in the
    rows of no triple.  Nothing else is written.  The gradient of E0 is P(G) + R: propagate G (`model._propagate(G)[0]`, the
    propagation is its own transpose) and add the regulariser's rows R with `bpr_reg_grad_` -- `decay` enters only there (here
    it is just checked).  return_coef=True appends coef [B] = sigmoid(x_j) / B.  Deterministic: repeated ids are summed in a
    fixed order, no atomics."""
    if not decay >= 0:
        raise ValueError("bpr_loss_grad: decay must be >= 0")
    users, pos, neg = _bpr_operands(M, E0, users, pos, neg, n_users)
    lib, st = _lib.load(), _lib.stream_ptr()
    B, n_items = users.numel(), E0.shape[0] - n_users
    dev = E0.device
    coef = torch.empty(B, dtype=torch.float32, device=dev)
    ws = torch.empty(2 * B, dtype=torch.float32, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    _bpr_loss(lib, M, E0, users, pos, neg, n_users, n_items, coef, ws, out2, None, st)
    G = torch.zeros(E0.shape, dtype=torch.float32, device=dev)
    _bpr_grad(lib, 0, _bpr_order(users, pos, neg, n_users), users, pos, neg, n_users, n_items, coef, M, G, 0.0, None, st)
    return (out2[0], out2[1], G, coef) if return_coef else (out2[0], out2[1], G)


@torch.no_grad()
def bpr_reg_grad_(D, E0, users, pos, neg, n_users, decay):
    """D[node] += (decay / B) * multiplicity * E0[node] for every node of the batch, in place: the gradient of decay * reg
    (the second half of `bpr_loss_grad`'s recipe).  Returns D."""
    users, pos, neg = _bpr_operands(D, E0, users, pos, neg, n_users)
    _bpr_grad(_lib.load(), 1, _bpr_order(users, pos, neg, n_users), users, pos, neg, n_users, E0.shape[0] - n_users, None, E0, D,
              float(decay) / users.numel(), None, _lib.stream_ptr())
    return D


class BPRTrainer:
    """The reference's training step (lightGCN.py:287-300) as HIP kernels around the propagation, for a single-GPU `LightGCN`:

        trainer = BPRTrainer(model, train_csr)          # batch_size 1024, lr 0.005, decay 1e-4: lightGCN.py:255-258
        mf, reg = trainer.step()                        # sample, loss, gradient, Adam

    train_csr: scipy CSR [n_users, n_items], sorted and de-duplicated once here (DeviceCSR) and kept on the device; every stored
    entry counts as an interaction, explicit zeros included.  A data_utils.DeviceCSR is taken as given: its constructor has
    done the same.
    The optimiser is FusedAdamW with weight_decay 0 (= torch.optim.Adam, as the reference).  step() enqueues, in order: one
    propagation, the loss kernel, the sort of the 3B (node, entry) pairs, the cotangent scatter, the propagation of the
    cotangent, the regulariser rows, the optimiser -- no autograd graph, no .item(), no host synchronisation; E0.grad holds
    the step's gradient afterwards.  The cotangent table G [N, d] is persistent: the regulariser pass clears the rows the
    scatter wrote.  (`_memset_G = True`, set by tools/bpr_step_probe.py only, zeroes the whole table every step instead: the
    variant the probe times against it, 0.450 against 0.445 ms per step at the Yelp shape: DESIGN.md §4.6c.)  The gradient
    table is a fresh one every step: `_propagate` allocates its result.

    Sampling differs from `sample_bpr_batch` in one point: only users with 0 < degree < n_items are ever drawn (the host
    sampler raises when it happens to draw a user without interactions and spins on one who has them all).  Users are drawn by
    a device torch.Generator (sorted; without replacement when at least batch_size are eligible, as lightGCN.py:231-238), items
    by gdmcf_bpr_sample_f32 with the count of draws as Philox offset.  `flag` (int32 [1] on the device; reading it
    synchronises) turns 1 when a step met an id out of range in device tensors handed to step() -- host arrays are
    range-checked before anything is enqueued.

    n_negs negatives per positive, neg_pool candidates per negative (`sample_bpr_negatives`; both 1: the step above, launch for
    launch).  batch_size stays the number of drawn (user, positive) pairs; a step then works on batch_size * n_negs triples --
    users and pos repeated n_negs times each (users stay sorted), neg flattened -- through the same loss, sort, scatter,
    regulariser and optimiser entries: mf is the mean of softplus over all of them and reg is `bpr_loss`'s with
    len(users) = batch_size * n_negs.  With neg_pool > 1 every negative is the candidate the current propagated table scores
    highest (dynamic negative sampling): step() propagates first and hands that one table to the sampler and to the loss.
    Both are construction arguments like batch_size: they are not in state_dict(), a resumed run passes the same ones."""

    def __init__(self, model, train_csr, batch_size=1024, lr=0.005, decay=1e-4, seed=0, n_negs=1, neg_pool=1):
        from .data_utils import DeviceCSR
        from .optim import FusedAdamW
        if model._world > 1:
            raise NotImplementedError("BPRTrainer: row-sharded (multi-GPU) models are not supported")
        E0 = model.E0.weight
        _lib.require_gpu(E0, "BPRTrainer: the model's E0")
        if batch_size < 1 or not decay >= 0:
            raise ValueError("BPRTrainer: batch_size >= 1 and decay >= 0 expected")
        if n_negs < 1 or neg_pool < 1:
            raise ValueError("BPRTrainer: n_negs >= 1 and neg_pool >= 1 expected")
        self.lib = _lib.load()
        dev = E0.device
        csr = train_csr if isinstance(train_csr, DeviceCSR) else DeviceCSR(train_csr, dev)
        if tuple(csr.shape) != (model.n_users, model.n_items):
            raise ValueError("BPRTrainer: train_csr must be [n_users, n_items] of the model")
        self.model, self.batch_size, self.decay, self.seed = model, int(batch_size), float(decay), int(seed)
        self.n_negs, self.neg_pool = int(n_negs), int(neg_pool)
        self.indptr, self.indices = csr.indptr.to(dev), csr.indices.to(dev)
        deg = self.indptr[1:] - self.indptr[:-1]
        self.eligible = torch.nonzero((deg > 0) & (deg < model.n_items)).reshape(-1)
        if self.eligible.numel() == 0:
            raise ValueError("BPRTrainer: no user has both an interacted and a non-interacted item")
        self.opt = FusedAdamW([E0], lr=lr, weight_decay=0.0)
        self.generator = torch.Generator(device=dev)
        self.generator.manual_seed(self.seed)
        self.steps = 0  # optimiser steps taken
        self.draws = 0  # batches sampled: the Philox offset of the next one
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.G = torch.zeros(E0.shape, dtype=torch.float32, device=dev)
        self._bufs = {}
        self._memset_G = False

    @torch.no_grad()
    def sample(self, M=None):
        """(users, pos, neg): int64 [batch_size * n_negs] on the device, users sorted; triple j * n_negs + k is drawn pair j with
        its k-th negative.  M: the propagated table the candidates of a pool are scored by (neg_pool > 1 only; propagated here
        when not given)."""
        B, n = self.batch_size, self.eligible.numel()
        dev = self.eligible.device
        if n >= B:
            pick = torch.randperm(n, generator=self.generator, device=dev)[:B]
        else:
            pick = torch.randint(0, n, (B,), generator=self.generator, device=dev)
        users = torch.sort(self.eligible[pick]).values
        pos = torch.empty_like(users)
        if self.n_negs == 1 and self.neg_pool == 1:
            neg = torch.empty_like(users)
            _bpr_sample(self.lib, self.indptr, self.indices, users, self.model.n_users, self.model.n_items, self.seed, self.draws,
                        pos, neg, self.flag, _lib.stream_ptr())
            self.draws += 1
            return users, pos, neg
        if self.neg_pool > 1 and M is None:
            M = self.model._propagate(self.model.E0.weight.detach())[0]
        neg = torch.empty(B * self.n_negs, dtype=torch.int64, device=dev)
        _bpr_sample_pool(self.lib, self.indptr, self.indices, users, self.n_negs, self.neg_pool, self.model.n_users,
                         self.model.n_items, M, self.seed, self.draws, pos, neg, self.flag, _lib.stream_ptr())
        self.draws += 1
        if self.n_negs > 1:
            users, pos = users.repeat_interleave(self.n_negs), pos.repeat_interleave(self.n_negs)
        return users, pos, neg

    def _ids(self, users, pos, neg):
        """The given triples as int64 device tensors; anything that lives on the host is range-checked there."""
        dev = self.G.device
        out = []
        for t, hi, what in ((users, self.model.n_users, "user"), (pos, self.model.n_items, "pos item"),
                            (neg, self.model.n_items, "neg item")):
            if t is None:
                raise ValueError("BPRTrainer.step: give users, pos and neg, or none of them")
            if not (torch.is_tensor(t) and t.is_cuda):
                t = torch.as_tensor(np.asarray(t.cpu() if torch.is_tensor(t) else t), dtype=torch.int64)
                if t.numel() and not (0 <= int(t.min()) and int(t.max()) < hi):
                    raise IndexError(f"BPRTrainer.step: {what} ids out of range")
            out.append(t.to(dev))
        return _bpr_operands(None, self.model.E0.weight, *out, self.model.n_users)

    @torch.no_grad()
    def step(self, users=None, pos=None, neg=None):
        """One optimiser step on the given triples (device tensors or host arrays; n_negs and neg_pool play no part), or on
        freshly sampled ones.  Returns (mf, reg): 0-d float32 device tensors, the two losses of `bpr_loss` before the update."""
        out2 = self._step(users, pos, neg)
        return out2[0], out2[1]

    @torch.no_grad()
    def train_epoch(self, n_steps):
        """n_steps calls of step() on freshly sampled triples: the body of the reference's epoch loop (lightGCN.py:285-304)
        without its .item() calls.  Returns (mean mf, mean reg) over the steps, 0-d float32 device tensors -- nothing
        synchronises."""
        if n_steps < 1:
            raise ValueError("BPRTrainer.train_epoch: n_steps >= 1 expected")
        mean = torch.stack([self._step() for _ in range(int(n_steps))]).mean(0)
        return mean[0], mean[1]

    @torch.no_grad()
    def _step(self, users=None, pos=None, neg=None):
        """step(), returning (mf, reg) as one float32 [2] device tensor"""
        m, lib = self.model, self.lib
        E0 = m.E0.weight
        M = None
        if users is None and pos is None and neg is None:
            if self.neg_pool > 1:  # the sampler scores its candidates by the table the loss reads: one propagation for both
                M = m._propagate(E0.detach())[0]
            users, pos, neg = self.sample(M)
        else:
            users, pos, neg = self._ids(users, pos, neg)
        st = _lib.stream_ptr()
        B, U, It = users.numel(), m.n_users, m.n_items
        coef, ws = self._bufs.get(B) or self._bufs.setdefault(B, (torch.empty(B, dtype=torch.float32, device=E0.device),
                                                                   torch.empty(2 * B, dtype=torch.float32, device=E0.device)))
        out2 = torch.empty(2, dtype=torch.float32, device=E0.device)  # (fresh: the caller may keep the losses of many steps)
        if M is None:
            M = m._propagate(E0.detach())[0]
        _bpr_loss(lib, M, E0, users, pos, neg, U, It, coef, ws, out2, self.flag, st)
        order = _bpr_order(users, pos, neg, U)
        if self._memset_G:
            self.G.zero_()
        try:
            _bpr_grad(lib, 0, order, users, pos, neg, U, It, coef, M, self.G, 0.0, None, st)
            D = m._propagate(self.G)[0]
            if D is self.G:  # (no layers: the propagation is the identity and returns its argument)
                D = self.G.clone()
            _bpr_grad(lib, 1, order, users, pos, neg, U, It, None, E0, D, self.decay / B, None if self._memset_G else self.G, st)
        except BaseException:
            self.G.zero_()  # the scattered rows must not leak into the next step's cotangent
            raise
        E0.grad = D
        self.opt.step()
        self.steps += 1
        return out2

    def state_dict(self):
        """Everything but the model: with `model.state_dict()` a run resumes bit-exactly."""
        return dict(optimizer=self.opt.state_dict(), steps=self.steps, draws=self.draws, seed=self.seed,
                    generator=self.generator.get_state())

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd["optimizer"])
        self.steps, self.draws, self.seed = int(sd["steps"]), int(sd["draws"]), int(sd["seed"])
        self.generator.set_state(sd["generator"])
