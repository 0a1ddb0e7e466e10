"""Which route a reverse loop takes ("Routes"): the one decision behind p_sample, recommend and driver.evaluate.
Host only -- no launch, no backbone module: every backbone class declares what its engine carries (`reverse_carries`), the
diffusion brings its tables, `plan` answers."""
import collections
import functools

import numpy as np
import torch

from . import _lib
from .engine_core import EpsTables

# What a backbone's engine carries.  latent: "base" -- the latent loop under latent=True and "extended"; "extended" -- under that alone;
# None -- none.  sparse_item: a binary CsrBatch stays sparse on the item-space loop (and the latent one); sparse_latent: on the latent
# route alone.  second_handle: the sparse latent loop takes the second branch's gathered pre-activation (onehot_rows_sparse).
Carries = collections.namedtuple("Carries", "latent sparse_item sparse_latent second_handle", defaults=(False, True))
_UNDECLARED = Carries(None, False)

# p_sample's answer: route "item" | "latent", a CsrBatch stays sparse, the EPSILON target's EpsTables on the latent route (else None).
# recommend's (None / False without masks): "item" | "latent" | "latent-csr", the loop ends at its last product's LatentProduct.
Plan = collections.namedtuple("Plan", "route keep_sparse eps recommend ends_at_product")


def carries(model):
    # Exact types: the declaration is read from the model's own class and is not inherited -- a subclass may change what the engine
    # was built for, so one that declares nothing takes the item route on dense rows.
    return vars(type(model)).get("reverse_carries", _UNDECLARED)


def latent_mode(latent):
    """The `latent` argument of p_sample / driver.evaluate / recommend (False / True / "extended") as None / "base" / "extended"."""
    if isinstance(latent, str) and latent == "extended":
        return "extended"
    return "base" if latent else None


class TableSet:
    """What the routes ask of one set of schedule tables; cached on the diffusion under the identity of _t32["c1"] / _t32["c2"] (`of`).
    One device read (x0_ok) and one gdmcf_schedule_build call (c1_0_positive, eps) per table set, each made when first asked for."""

    def __init__(self, c1, c2, host_tables):
        self.c1, self.c2, self._host_tables = c1, c2, host_tables

    @staticmethod
    def of(diffusion):
        c1, c2 = diffusion._t32.get("c1"), diffusion._t32.get("c2")
        rec = getattr(diffusion, "_route_tables", None)
        if rec is None or rec.c1 is not c1 or rec.c2 is not c2:
            rec = diffusion._route_tables = TableSet(c1, c2, diffusion._host_tables)
        return rec

    @functools.cached_property
    def x0_ok(self):
        """posterior_mean_coef2[0] == 0 (alphas_cumprod_prev[0] is 1 for every schedule: the last step needs no x_1) and finite
        posterior_mean_coef1, as float32 on the device."""
        return (self.c1 is not None and self.c2 is not None and bool(self.c2[0].item() == 0.0)
                and bool(torch.isfinite(self.c1).all().item()))

    @functools.cached_property
    def _host(self):
        """(c1_0_positive, eps) from the host's float64 tables, rounded to float32 first as the item-space route reads them (no device
        read): posterior_mean_coef1[0] > 0 (recommend ranks raw scores); the EPSILON target's EpsTables, whose `ok` every plan reads."""
        tabs = self._host_tables()
        c1, c2, r1, r2 = (tabs[_lib.TABLE_NAMES.index(name)].astype("float32") for name in (
            "posterior_mean_coef1", "posterior_mean_coef2", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"))
        return bool(np.isfinite(c1[0]) and c1[0] > 0), EpsTables(c1, c2, r1, r2, len(c1))

    c1_0_positive = property(lambda self: self._host[0])
    eps = property(lambda self: self._host[1])


def plan(diffusion, model, rows, steps, sampling_noise=False, capture=None, mode=None, masks=None):
    """The Plan of one reverse loop.  rows: dense tensor, CsrBatch or DeviceCSR; mode: latent_mode(); masks: None for p_sample, the
    tuple of DeviceCSRs recommend masks with.
    Latent route: the loop must be linear in x_t between two hidden activations -- no sampling noise, no F.normalize, no active
    dropout, float32 products -- nothing may ask for the per-step x_t (capture), the backbone's engine has the loop under this mode,
    and the tables allow it: x0 target, c2[0] == 0 (x0_ok); under "extended" also the EPSILON target, finite g, d, G, D > 0 (eps).
    Sparse rows: x_T must be x_0 itself (steps == 0), binary and undropped, so that the first layers' products are sums of weight
    rows.  recommend: the latent route from the binary rows ("latent-csr") or dense ones ("latent") where c1[0] > 0 (x0: raw scores
    are ranked); the EPSILON target's x_0 = G x_T - D (...) is ranked without its first term only where `rows` is among `masks`."""
    car, tabs = carries(model), TableSet.of(diffusion)
    target = getattr(diffusion.mean_type, "name", None)
    x0 = target == "START_X"
    plain = (diffusion.noise_scale != 0.0 and not model.norm and (not model.training or model.drop.p == 0)
             and getattr(model, "gemm_dtype", "f32") == "f32")
    latent = bool(mode is not None and plain and not sampling_noise and capture is None and car.latent in ("base", mode)
                  and (x0 or (mode != "base" and target == "EPSILON"))
                  and (tabs.x0_ok if x0 else tabs.c1 is not None and tabs.eps.ok))
    binary = steps == 0 and not isinstance(rows, torch.Tensor) and getattr(rows, "csr", rows).values is None
    keep_sparse = bool(binary and plain and (car.sparse_item or (latent and car.sparse_latent)))
    recommend = None
    if masks is not None:
        if not latent or (x0 and not tabs.c1_0_positive):
            recommend = "item"
        else:
            recommend = "latent-csr" if binary and (x0 or any(m is rows for m in masks)) else "latent"
    return Plan("latent" if latent else "item", keep_sparse, tabs.eps if latent and not x0 else None, recommend,
                recommend == "latent-csr" or (recommend == "latent" and x0))
