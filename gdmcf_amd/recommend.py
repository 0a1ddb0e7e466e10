"""`recommend`: ranked top-k items per user id for the diffusion models, in one call, from rows that stay on the device
(DESIGN 4.10).  What `driver.evaluate` does per batch -- reverse loop, history mask, top-k (reference main.py:288-301) -- with the
mask rows picked on the device by user id (gdmcf_topk_masked_rows_f32) and, where the reverse loop runs in the first hidden
layer's space, without the dense x_T, the posterior epilogue and x_0 itself: the top-k is invariant under the positive factor
c1[0], so the raw scores of the last product are ranked and only the k returned values are scaled."""
import numpy as np
import torch

from . import _lib
from . import engine_core as core
from .data_utils import DeviceCSR


def _c1_0_positive(diffusion):
    """posterior_mean_coef1[0] > 0 as float32, from the host's float64 table (gdmcf_schedule_build; no device read); once per
    table set."""
    c1 = diffusion._t32.get("c1")
    rec = getattr(diffusion, "_recommend_c1_rec", None)
    if rec is None or rec[0] is not c1:
        from .gaussian_diffusion import _SCHEDULE_KIND
        tabs = _lib.schedule_tables(_SCHEDULE_KIND[diffusion.noise_schedule], diffusion.noise_scale, diffusion.noise_min,
                                    diffusion.noise_max, diffusion.steps, diffusion.beta_fixed)
        c1_0 = np.float32(tabs[_lib.TABLE_NAMES.index("posterior_mean_coef1")][0])
        rec = diffusion._recommend_c1_rec = (c1, bool(np.isfinite(c1_0) and c1_0 > 0))
    return rec[1]


def route_of(diffusion, model, rows, sampling_steps=0, sampling_noise=False, extended=False, masks=None):
    """Which route `recommend` takes for this call:
      "latent-csr"  GaussianDiffusion._latent_reverse_ok holds (x0 target, no sampling noise, no F.normalize, no active dropout,
                    float32 products, DNN / DNNOneHot / DNNOneHotEmbedding / DNNOneHotEmbeddingGCN), sampling_steps == 0 and every
                    value of `rows` is 1: gathered first layers, latent steps, one item-wide product, top-k on the raw scores
      "latent"      _latent_reverse_ok holds but x_T is not the binary rows (sampling_steps > 0, values other than 1): the same,
                    from dense rows
      "item"        everything else: p_sample as driver.evaluate calls it, then the top-k.
    extended (recommend(latent="extended")): _latent_reverse_ok(extended=True) decides, so DNNCat takes the same two routes, and
    so does the EPSILON target with one more condition on "latent-csr": x_0 = G x_T - D (second Q^ + b_out) is ranked without
    its first term, which is only right where G x_T touches masked items alone -- `rows` itself must be among `masks` (the
    tuple of DeviceCSRs the call masks with); otherwise "latent" (dense rows, x_0 from the posterior epilogue)."""
    if not extended:
        if not (diffusion._latent_reverse_ok(model, sampling_noise, None) and _c1_0_positive(diffusion)):
            return "item"
        return "latent-csr" if (sampling_steps == 0 and rows.values is None) else "latent"
    if not diffusion._latent_reverse_ok(model, sampling_noise, None, extended=True):
        return "item"
    from .gaussian_diffusion import ModelMeanType
    eps = diffusion.mean_type == ModelMeanType.EPSILON
    if not eps and not _c1_0_positive(diffusion):
        return "item"
    binary = sampling_steps == 0 and rows.values is None
    if eps:
        return "latent-csr" if binary and masks is not None and any(m is rows for m in masks) else "latent"
    return "latent-csr" if binary else "latent"


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


def recommend(diffusion, model, rows, user_ids, k, *, mask="rows", sampling_steps=0, sampling_noise=False, batch_size=400,
              return_values=False, noise0=None, sampled0=None, latent=True):
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
    latent: True -- the routes above; "extended" -- route_of(extended=True): DNNCat on both latent routes, and the EPSILON
    target: on "latent-csr" (only with `rows` itself among the masks) second (-Q^) + (-b_out) is ranked and the k values scaled by
    D; on "latent" x_0 comes from the posterior epilogue on dense rows and is ranked as it is."""
    if not isinstance(rows, DeviceCSR):
        raise TypeError("gdmcf_amd.recommend: rows must be a gdmcf_amd.data_utils.DeviceCSR")
    _lib.require_gpu(rows.indptr, "rows")
    masks = _as_mask(mask, rows)
    for m in masks:
        _lib.require_gpu(m.indptr, "mask")
    dev, (U, I) = rows.device, rows.shape
    k, batch_size = int(k), int(batch_size)
    if not 1 <= k <= I:
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
    n = ids.numel()
    if not (latent is True or (isinstance(latent, str) and latent == "extended")):
        raise ValueError('recommend: latent is True or "extended"')
    extended = latent is not True
    route = route_of(diffusion, model, rows, sampling_steps, sampling_noise, extended=extended, masks=masks)
    diffusion.last_recommend_route = route
    from .gaussian_diffusion import ModelMeanType
    # the EPSILON target's x_0 = G x_T + D (second (-Q^) + (-b_out)): where G x_T lies on masked items only ("latent-csr") the bracket
    # is ranked like the x0 target's last product; on "latent" x_0 itself comes from the posterior epilogue on dense rows
    stop = route == "latent-csr" or diffusion.mean_type != ModelMeanType.EPSILON
    idx = torch.empty(n, k, dtype=torch.int64, device=dev)
    val = torch.empty(n, k, dtype=torch.float32, device=dev) if return_values else None
    if n == 0:
        return (val, idx) if return_values else idx
    lib, eng = _lib.load(), model.engine
    ip1, ix1 = (masks[0].indptr, masks[0].indices) if masks else (None, None)
    ip2, ix2 = (masks[1].indptr, masks[1].indices) if len(masks) > 1 else (None, None)
    for lo in range(0, n, batch_size):
        chunk = ids[lo:lo + batch_size]
        B = chunk.numel()
        index = chunk if getattr(diffusion, "indexIn", False) else None
        scale = None
        inj = {name: t[lo:lo + B].to(dev) for name, t in (("noise0", noise0), ("sampled0", sampled0)) if t is not None}
        if route == "item":
            kw = dict(inj, index=index) if index is not None else inj
            scores = core._f32_rows(diffusion.p_sample(model, rows.rows(chunk), sampling_steps, sampling_noise, **kw))
        else:
            x = rows.batch(chunk) if route == "latent-csr" else rows.rows(chunk)
            res = diffusion._latent_sample(model, x, sampling_steps, index, stop=stop, **inj)  # (as p_sample(latent=...) runs it)
            if stop:  # the last product's raw scores are ranked, the k returned values scaled
                scores, scale = eng.score_product(res.A, res.second, res.K, res.bias, B, dev), res.scale
            else:
                scores = res
            diffusion.last_reverse_route = "latent"
        v = val[lo:lo + B] if val is not None else None
        _lib.check(lib.gdmcf_topk_masked_rows_f32(
            scores.data_ptr(), scores.stride(0), B, I, _lib.ptr(ip1), _lib.ptr(ix1), _lib.ptr(ip2), _lib.ptr(ix2),
            chunk.data_ptr(), _lib.ptr(scale), k, idx[lo:lo + B].data_ptr(), _lib.ptr(v), _lib.stream_ptr()))
    return (val, idx) if return_values else idx
