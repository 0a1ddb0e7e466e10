"""`recommend`: ranked top-k items per user id for the diffusion models, in one call, from rows that stay on the device
(DESIGN 4.10).  What `driver.evaluate` does per batch -- reverse loop, history mask, top-k (reference main.py:288-301) -- with the
mask rows picked on the device by user id (gdmcf_topk_masked_rows_f32) and, where the reverse loop runs in the first hidden
layer's space, without the dense x_T, the posterior epilogue and x_0 itself: the top-k is invariant under the positive factor
c1[0], so the raw scores of the last product are ranked and only the k returned values are scaled.
`score_candidates` / `recommend(candidates=)`: the same call for the items a caller names per user -- where the
reverse loop ends at the operands of its last product and the lists are short, only the named rows of the output weight are
read (gdmcf_cand_scores_f32); otherwise the named scores are picked out of the [B, I] ones (gdmcf_cand_pick_f32).
`rank_targets`: the same call ending in the exact rank of every item a target matrix names per user, in that order,
instead of a list (gdmcf_rank_targets_f32) -- the evaluation side: every metric that is a function of where the held-out items sit."""
import types

import torch

from . import _lib, reverse_route
from . import engine_core as core
from .data_utils import DeviceCSR


def route_of(diffusion, model, rows, sampling_steps=0, sampling_noise=False, extended=False, masks=None):
    """Which route `recommend` takes for this call (reverse_route.plan decides; DESIGN 4.9, "Routes"; extended: latent="extended"):
      "latent-csr"  the latent loop from the binary rows themselves: gathered first layers, one item-wide product, raw scores ranked
      "latent"      the latent loop from dense rows (sampling_steps > 0, values other than 1, or the EPSILON target without `rows`
                    among `masks`, the tuple of DeviceCSRs the call masks with)
      "item"        everything else: p_sample as driver.evaluate calls it, then the top-k."""
    return reverse_route.plan(diffusion, model, rows, sampling_steps, sampling_noise, None, "extended" if extended else "base",
                              masks or ()).recommend


def _as_mask(mask, rows):
    if mask is None:
        return ()
    if isinstance(mask, str):
        if mask != "rows":
            raise ValueError('recommend: mask is "rows", None, a DeviceCSR or a pair of DeviceCSRs')
        return (rows,)
    masks = (mask,) if isinstance(mask, DeviceCSR) else tuple(mask)
    if not 1 <= len(masks) <= 2 or not all(isinstance(m, DeviceCSR) for m in masks):
        raise ValueError('recommend: mask is "rows", None, a DeviceCSR or a pair of DeviceCSRs')
    return masks


CANDIDATE_ROUTES = ("auto", "gathered", "picked")


def candidate_route_of(B, C, I, has_product):
    """Which entry scores a chunk of B users with C candidates each out of I items: "gathered" (gdmcf_cand_scores_f32 on the
    operands of the last product) where the reverse loop ended at a LatentProduct and B * C <= I, "picked" (the [B, I] scores,
    then gdmcf_cand_pick_f32) otherwise.  The rule is derived, not measured: the gathered bytes B C K 4 do not exceed one pass
    over the output weight, I K 4 -- conservative, because the full product is bound by its MFMAs above its bytes."""
    return "gathered" if has_product and int(B) * int(C) <= int(I) else "picked"


def _as_candidates(candidates, n, k=None, candidate_route="auto"):
    """The candidate lists as an int64 tensor [n, C] or [C] (still where the caller keeps them); the argument errors of a call
    with candidates."""
    if candidate_route not in CANDIDATE_ROUTES:
        raise ValueError('recommend: candidate_route is "auto", "gathered" or "picked"')
    cand = torch.as_tensor(candidates)
    if cand.dtype.is_floating_point or cand.dtype == torch.bool or cand.is_complex():
        raise TypeError("recommend: candidates must be integers")
    if cand.dim() not in (1, 2):
        raise ValueError("recommend: candidates is [n, C], aligned with user_ids, or one shared list [C]")
    if cand.dim() == 2 and cand.shape[0] != n:
        raise ValueError(f"recommend: candidates has {cand.shape[0]} rows for {n} user ids")
    C = cand.shape[-1]
    if C < 1:
        raise ValueError("recommend: candidates holds no item")
    if k is not None and not 1 <= int(k) <= C:
        raise AssertionError("selected index k out of range")
    return cand.to(torch.int64)


def _setup(diffusion, model, rows, user_ids, mask, sampling_steps, sampling_noise, batch_size, latent, k=None):
    """What recommend and score_candidates share ahead of their chunks: the checks (k: against the item count), the ids on the
    device, the route."""
    _lib.require_gpu(rows.indptr, "rows")
    masks = _as_mask(mask, rows)
    for m in masks:
        _lib.require_gpu(m.indptr, "mask")
    dev, (U, I) = rows.device, rows.shape
    batch_size = int(batch_size)
    if k is not None and not 1 <= k <= I:
        raise AssertionError("selected index k out of range")
    if batch_size < 1:
        raise ValueError("recommend: batch_size must be positive")
    ids = torch.as_tensor(user_ids, dtype=torch.int64).reshape(-1)
    n_ok = min([U] + [m.shape[0] for m in masks])
    if ids.numel():  # (a device tensor costs one synchronising copy per call here; a host sequence none)
        lo, hi = torch.aminmax(ids)
        if not (0 <= int(lo) and int(hi) < n_ok):
            raise IndexError("recommend: user_ids out of range")
    ids = ids.to(dev).contiguous()
    if latent is not True and reverse_route.latent_mode(latent) in (None, "base"):
        raise ValueError('recommend: latent is True or "extended"')
    # (has_product -- the EPSILON target's "latent" route has none: x_0 itself comes from the posterior epilogue on dense rows)
    plan = diffusion._reverse_plan(model, rows, sampling_steps, sampling_noise, None, latent, masks)  # (sets last_reverse_route)
    diffusion.last_recommend_route = plan.recommend
    ip1, ix1 = (masks[0].indptr, masks[0].indices) if masks else (None, None)
    ip2, ix2 = (masks[1].indptr, masks[1].indices) if len(masks) > 1 else (None, None)
    return types.SimpleNamespace(dev=dev, I=I, ids=ids, n=ids.numel(), batch_size=batch_size, route=plan.recommend, plan=plan,
                                 masks=masks, has_product=plan.ends_at_product, sampling_steps=sampling_steps,
                                 sampling_noise=sampling_noise, mask_ptrs=tuple(_lib.ptr(t) for t in (ip1, ix1, ip2, ix2)))


def _reverse_chunks(diffusion, model, rows, c, noise0=None, sampled0=None):
    """The reverse loop of every chunk of c.batch_size users: (lo, chunk, B, product, scores) with either the
    engine_core.LatentProduct the loop ended at (c.has_product) or the [B, I] float32 predictions."""
    dev = c.dev
    for lo in range(0, c.n, c.batch_size):
        chunk = c.ids[lo:lo + c.batch_size]
        B = chunk.numel()
        index = chunk if getattr(diffusion, "indexIn", False) else None
        inj = {name: t[lo:lo + B].to(dev) for name, t in (("noise0", noise0), ("sampled0", sampled0)) if t is not None}
        if c.route == "item":
            kw = dict(inj, index=index) if index is not None else inj
            yield lo, chunk, B, None, core._f32_rows(diffusion.p_sample(model, rows.rows(chunk), c.sampling_steps, c.sampling_noise, **kw))
            continue
        x = rows.batch(chunk) if c.route == "latent-csr" else rows.rows(chunk)
        res = diffusion._latent_sample(model, x, c.sampling_steps, index, c.has_product, c.plan.eps, **inj)
        yield (lo, chunk, B, res, None) if c.has_product else (lo, chunk, B, None, res)


def _all_scores(eng, B, dev, product, scores):
    """([B, I] scores, scale or None): the last product's raw scores where the loop ended at its operands (they are ranked, the
    returned values scaled), the predictions as they are otherwise."""
    if product is None:
        return scores, None
    return eng.score_product(product.A, product.second, product.K, product.bias, B, dev), product.scale


def _score_chunk(diffusion, eng, c, cand, lo, chunk, B, product, scores, out, candidate_route):
    """out[B, C] = the scores of the chunk's candidates, -inf for masked and out-of-range ones (one launch on "gathered", the
    item-wide scores and one launch on "picked")."""
    shared = cand.dim() == 1
    cc = cand if shared else cand[lo:lo + B]
    C, ldcand = cc.shape[-1], 0 if shared else cc.stride(0)
    how = candidate_route_of(B, C, c.I, product is not None) if candidate_route == "auto" else candidate_route
    if how == "gathered":
        core.cand_scores(eng.lib, product.A, product.second, c.I, product.K, product.bias, product.scale, cc, ldcand, B, C,
                         c.mask_ptrs, chunk, out, _lib.stream_ptr())
    else:
        scores, scale = _all_scores(eng, B, c.dev, product, scores)
        core.cand_pick(eng.lib, scores, B, c.I, scale, cc, ldcand, C, c.mask_ptrs, chunk, out, _lib.stream_ptr())
    diffusion.last_candidate_route = how


def _check_candidate_route(c, candidate_route):
    if candidate_route == "gathered" and not c.has_product:
        raise ValueError(f'recommend: candidate_route="gathered" needs a reverse loop that ends at the operands of its last '
                         f'product; this call takes the "{c.route}" route' + ("" if c.route == "item" else " with the EPSILON target"))


def score_candidates(diffusion, model, rows, user_ids, candidates, *, mask="rows", sampling_steps=0, sampling_noise=False,
                     batch_size=400, latent=True, candidate_route="auto", noise0=None, sampled0=None):
    """The predictions [n, C] (float32, on the device, in candidate order) of the items `candidates` names for the users
    `user_ids` of the DeviceCSR `rows`: what a re-ranker, an allow-list or the sampled-negatives protocol asks of the model.

    candidates: an integer tensor or sequence, [n, C] aligned with user_ids or [C] shared by all of them; uploaded once, as
    int64.  A candidate in the user's mask rows, or outside [0, I) (-1 pads a ragged list), scores -inf; a duplicate is scored
    each time it occurs.  Routes, masks, `index`, the injected draws and the chunks are recommend's.
    Per chunk of B users, `diffusion.last_candidate_route` names what ran (candidate_route_of):
      "gathered"  the reverse loop ended at the operands of its last product (route "latent-csr", or "latent" without the EPSILON
                  target) and B * C <= I: gdmcf_cand_scores_f32 reads the C named rows of the output weight per user -- no
                  item-wide product, no [B, I] buffer;
      "picked"    otherwise: the [B, I] scores as recommend forms them, then gdmcf_cand_pick_f32.
    candidate_route="gathered" / "picked" forces the choice ("gathered" without such a loop: ValueError).  The values are the
    predictions themselves (scaled by c1[0], or D, on the latent routes), within float32 rounding of p_sample's x_0."""
    if not isinstance(rows, DeviceCSR):
        raise TypeError("gdmcf_amd.score_candidates: rows must be a gdmcf_amd.data_utils.DeviceCSR")
    user_ids = torch.as_tensor(user_ids, dtype=torch.int64).reshape(-1)  # (converted once: _setup takes the tensor as it is)
    cand = _as_candidates(candidates, user_ids.numel(), None, candidate_route)
    c = _setup(diffusion, model, rows, user_ids, mask, sampling_steps, sampling_noise, batch_size, latent)
    _check_candidate_route(c, candidate_route)
    cand = cand.to(c.dev).contiguous()
    out = torch.empty(c.n, cand.shape[-1], dtype=torch.float32, device=c.dev)
    for lo, chunk, B, product, scores in _reverse_chunks(diffusion, model, rows, c, noise0, sampled0):
        _score_chunk(diffusion, model.engine, c, cand, lo, chunk, B, product, scores, out[lo:lo + B], candidate_route)
    return out


def recommend(diffusion, model, rows, user_ids, k, *, mask="rows", sampling_steps=0, sampling_noise=False, batch_size=400,
              return_values=False, noise0=None, sampled0=None, latent=True, candidates=None, candidate_route="auto"):
    """Top-k item ids [n, k] (int64, on the device; with return_values: (values [n, k] float32, ids)) for the users `user_ids` of
    the DeviceCSR `rows`: the reverse loop from each user's row, the mask's items set to -inf, the k largest predictions in
    descending order, equal ones in ascending item index (evaluate_utils.masked_topk's conventions).

    user_ids: int64 tensor or sequence, any order, repeats allowed; uploaded once.  mask: "rows" (the same matrix, as the
    reference's evaluation), None, a DeviceCSR, or a pair of them (both are masked: train + valid without a summed matrix).
    The users are worked in chunks of `batch_size`; per chunk only launches are enqueued -- no scipy slicing, no copy from the
    host, no synchronisation.  `diffusion.last_recommend_route` names the route (route_of).  On the two latent routes the values
    are c1[0] times the raw scores of the last product, within float32 rounding of p_sample's x_0; on the "item" route values and
    ids are masked_topk(p_sample(...))'s bits.  With `diffusion.indexIn` the chunk's ids are the model's `index`.
    The ids are range-checked once per call (the kernels do not check them): on the host for a host sequence; ids that already
    live on the device cost the call's one synchronising copy there.
    noise0 [n, I] / sampled0 [n, I] inject the draws of x_T with sampling_steps > 0, row for row of user_ids, as p_sample's
    keywords of the same names do (parity runs).
    latent: True or "extended" (DNNCat and the EPSILON target on the latent routes too: DESIGN 4.9, "Routes").  With the EPSILON
    target "latent-csr" ranks second (-Q^) + (-b_out) and scales the k values by D; "latent" ranks the posterior epilogue's x_0.
    candidates (score_candidates' lists, [n, C] or a shared [C]; candidate_route as there): only these items are ranked, 1 <= k
    <= C.  The ids returned are the candidates' item ids; equal scores come back in ascending POSITION in the list (the top-k
    runs over list positions, which one torch.gather translates); return_values returns the scores; masked or out-of-range
    candidates appear, with -inf, only when fewer than k candidates are live; a candidate listed twice can appear twice.
    With candidates=None nothing of this runs."""
    if not isinstance(rows, DeviceCSR):
        raise TypeError("gdmcf_amd.recommend: rows must be a gdmcf_amd.data_utils.DeviceCSR")
    k = int(k)
    cand = None
    if candidates is not None:
        user_ids = torch.as_tensor(user_ids, dtype=torch.int64).reshape(-1)  # (converted once: _setup takes the tensor as it is)
        cand = _as_candidates(candidates, user_ids.numel(), k, candidate_route)
    c = _setup(diffusion, model, rows, user_ids, mask, sampling_steps, sampling_noise, batch_size, latent,
               k if cand is None else None)  # (with candidates k is bounded by C, which duplicates may take past I)
    dev, n, I = c.dev, c.n, c.I
    idx = torch.empty(n, k, dtype=torch.int64, device=dev)
    val = torch.empty(n, k, dtype=torch.float32, device=dev) if return_values else None
    if cand is not None:
        _check_candidate_route(c, candidate_route)
        cand = cand.to(dev).contiguous()
    if n == 0:
        return (val, idx) if return_values else idx
    lib, eng = _lib.load(), model.engine
    for lo, chunk, B, product, scores in _reverse_chunks(diffusion, model, rows, c, noise0, sampled0):
        v = val[lo:lo + B] if val is not None else None
        if cand is not None:
            C = cand.shape[-1]
            picked = torch.empty(B, C, dtype=torch.float32, device=dev)
            _score_chunk(diffusion, eng, c, cand, lo, chunk, B, product, scores, picked, candidate_route)
            pos = idx[lo:lo + B]
            _lib.check(lib.gdmcf_topk_masked_f32(picked.data_ptr(), picked.stride(0), B, C, None, None, k, pos.data_ptr(),
                                                 _lib.ptr(v), _lib.stream_ptr()))
            pos.copy_(torch.gather(cand.expand(B, C) if cand.dim() == 1 else cand[lo:lo + B], 1, pos))  # positions -> item ids
            continue
        scores, scale = _all_scores(eng, B, dev, product, scores)
        _lib.check(lib.gdmcf_topk_masked_rows_f32(
            scores.data_ptr(), scores.stride(0), B, I, *c.mask_ptrs, chunk.data_ptr(), _lib.ptr(scale), k,
            idx[lo:lo + B].data_ptr(), _lib.ptr(v), _lib.stream_ptr()))
    return (val, idx) if return_values else idx


def rank_targets(diffusion, model, rows, user_ids, targets, *, mask="rows", sampling_steps=0, sampling_noise=False, batch_size=400,
                 latent=True, noise0=None, sampled0=None, return_live=False):
    """The exact catalogue ranks [n, G] (int32, on the device) of the items the DeviceCSR `targets` names per user -- an
    evaluation's held-out items -- in the order `recommend` ranks by: ranks[r, j] is the number of items that precede the j-th
    entry of row user_ids[r] of `targets` when the mask's items count as -inf, larger predictions come first and equal ones in
    ascending item index; the 0-based place the item has in recommend(..., k = I)'s list (gdmcf_rank_targets_f32).  Every
    quantity that is a function of where the held-out items sit follows from it without a [n, I] copy to the host: untruncated
    MRR, mean rank, Recall@N for an N chosen afterwards, leave-one-out HR@N / NDCG@N (evaluate_utils.rank_metrics_device), and with
    return_live percentiles and AUC.

    targets: a DeviceCSR with `rows`' shape (its values are not read).  G = targets.max_row_len (at least 1); columns past the
    length of a user's row hold -1.  A masked target is ranked inside the -inf tail by its index, as the top-k would list it.
    return_live: (ranks, n_live [n] int32) -- the number of unmasked items per user.
    Everything else is recommend's: the routes (`diffusion.last_recommend_route`; on the latent routes the raw scores of the
    last product are ranked, which the positive scale does not reorder), masks, chunks of `batch_size`, `index`, the injected
    draws noise0 / sampled0, the id checks.  Per chunk one launch follows the scores; no top-k runs and nothing synchronises.
    Candidate lists are not taken: a rank inside a [n, C] list is two torch operations on score_candidates' output s,
    (s > s.gather(1, pos)).sum(1) plus the equal scores at lower positions."""
    if not isinstance(rows, DeviceCSR):
        raise TypeError("gdmcf_amd.rank_targets: rows must be a gdmcf_amd.data_utils.DeviceCSR")
    if not isinstance(targets, DeviceCSR):
        raise TypeError("gdmcf_amd.rank_targets: targets must be a gdmcf_amd.data_utils.DeviceCSR")
    if tuple(targets.shape) != tuple(rows.shape):
        raise ValueError(f"gdmcf_amd.rank_targets: targets has shape {tuple(targets.shape)}, rows {tuple(rows.shape)}")
    c = _setup(diffusion, model, rows, user_ids, mask, sampling_steps, sampling_noise, batch_size, latent)
    _lib.require_gpu(targets.indptr, "targets")
    dev, n, I = c.dev, c.n, c.I
    G = max(int(targets.max_row_len), 1)
    ranks = torch.empty(n, G, dtype=torch.int32, device=dev)
    live = torch.empty(n, dtype=torch.int32, device=dev) if return_live else None
    if n:
        lib, eng = _lib.load(), model.engine
        # (a matrix without any entry: an empty tensor has no pointer, and no indptr range covers the one index handed over instead)
        tix = targets.indices if targets.indices.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        for lo, chunk, B, product, scores in _reverse_chunks(diffusion, model, rows, c, noise0, sampled0):
            scores, _ = _all_scores(eng, B, dev, product, scores)
            _lib.check(lib.gdmcf_rank_targets_f32(
                scores.data_ptr(), scores.stride(0), B, I, *c.mask_ptrs, targets.indptr.data_ptr(), tix.data_ptr(),
                chunk.data_ptr(), G, ranks[lo:lo + B].data_ptr(), ranks.stride(0),
                _lib.ptr(live[lo:lo + B]) if live is not None else None, _lib.stream_ptr()))
    return (ranks, live) if return_live else ranks
