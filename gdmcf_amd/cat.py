"""Backbone `DNNCat` (reference models/DNN.py:180-265) on the HIP path: the plain `DNN` with one learnable layer in front,
`cat_layer = Linear(3, 1)`, which mixes per user x item the noised value x_t[b,i] with the item's two one-hot columns
x_U[b,i,0:2] into one scalar; dropout, the time embedding and the MLP follow unchanged.  It is driven by
`GaussianDiffusionDiscrete(CatOneHot=True)` with `indexIn` off, like `DNNOneHot`, and reads the same [B, 2I] one-hot image
(`gdmcf_onehot_noise_f32`).

Downstream of the mix this is `DenoiserEngine`'s layer chain.  Two things differ (csrc/cat.hip):
  * the input step: `gdmcf_cat_prep_input_f32` forms x_t, the mix and the dropout in one pass and writes the first layer's input
    and x_t -- no [B, I, 3] tensor, no element-wise passes in front of the first GEMM;
  * the tail of the backward pass: the first layer's input is a function of parameters, so dxin = dZ1 . W1[:, 0:I]
    (`gdmcf_linear_bwd_input_f32` on the first I columns of W1, its leading dimension) and `gdmcf_cat_grad_f32`, which reduces
    it to cat_layer's four gradients.  The keep-mask is recomputed there from the builder's Philox position, not stored.

Rows that stay sparse (opt-in: `DNNCat(..., csr_rows=True)`): a `data_utils.CsrBatch` (x0 target, all values 1, Philox or given
noise) then feeds `gdmcf_cat_prep_input_csr_f32` -- densify, class draws and the builder in one launch, the rows and the classes
left as two bitmaps -- the loss takes its target from the row bitmap and `gdmcf_cat_grad_bits_f32` the one-hot pair from both;
no dense batch and no [B, 2I] image exist (the image's buffer is made by the first DENSE training step only).  The Philox
positions are the dense route's and both kernels' outputs are the dense ones' bit for bit, so a run on `csr.batch(ids)` is the
run on `csr.rows(ids)`.  The default stays
`csr_rows=False` (`training_losses` densifies a CsrBatch, as it does for every configuration the sparse kernels do not cover:
eps target, values other than 1, torch-drawn noise).

Not built (each raises NotImplementedError): `norm=True`, GEMM inputs other than f32, AdamW fused into the backward pass
(dxin reads W1: the first layer's update must not run before it), the graphed step, data parallel; the item-space
reverse loop takes dense rows only (the latent one, `p_sample(latent="extended")`, also binary CSR rows: CatEngine.latent_loop).  Constructor, parameter names and initialisation draw order are the reference's, so checkpoints interchange.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import engine_core as core
from .engine import DenoiserEngine
from .engine_core import _Bufs, with_precision
from .onehot import OneHotEngine
from .reverse_route import Carries


class CatEngine(DenoiserEngine):
    supports_grad_sink = False  # (data parallel is not extended to this backbone)

    onehot_rows = OneHotEngine.onehot_rows  # x_tU as the [B, 2I] float image (gdmcf_onehot_noise_f32)
    _last_layer = OneHotEngine._last_layer  # output layer, plain or with the posterior mean in its epilogue
    _xU = OneHotEngine._xU  # bufs.xU, the [B, 2I] image of the dense route, made on its first step

    def buffers(self, B, device):
        b = super().buffers(B, device)
        if getattr(b, "dxin", None) is None:
            f32 = dict(dtype=torch.float32, device=device)
            b.xU = None  # never made by a run on CSR rows (_xU)
            b.x0bits = b.clsbits = None  # the sparse route's rows and classes as bitmaps (_train_input_csr)
            b.xt = torch.zeros(B, b.ldi, **f32)  # x_t: eps target, posterior, and the backward pass's first sum
            b.dxin = torch.zeros(B, b.ldi, **f32)
            b.cat_ws_bytes = int(self.lib.gdmcf_cat_grad_ws_bytes(B, self.I))
            b.cat_ws = torch.empty(max(b.cat_ws_bytes, 256), dtype=torch.uint8, device=device)
            self._grow_workspace(b, B, device, [(self.model.in_layers[0].weight.shape[0], self.I)])  # the dxin product
        return b

    # -- input step -----------------------------------------------------------------------------------------------------
    def _cat_input(self, bufs, x, xU, ts, ca, cb, noise, drop_mask, training):
        """gdmcf_cat_prep_input_f32 at the next Philox position: bufs.xin = [ drop(cat_layer(x_t, xU)) | emb(t) | 1 | 0-pad ],
        bufs.xt = x_t.  Remembers the dropout's (mode, mask, p, position) for the backward pass; returns what the kernel
        reads, to keep referenced."""
        m = self.model
        B = x.shape[0]
        x = core._f32_rows(x)
        p = float(m.drop.p)
        noise_mode, noise, drop_mode, keep = core._prep_modes(B, ca, noise, drop_mask, p, training)
        (nz, ldn), (kp, ldkp) = core._pl(noise), core._pl(keep)
        cw, cb_ = self._cat_params()
        self.offset += 1
        _lib.check(self.lib.gdmcf_cat_prep_input_f32(
            x.data_ptr(), x.stride(0), xU.data_ptr(), xU.stride(0), ts.data_ptr(), _lib.ptr(ca), _lib.ptr(cb), noise_mode, nz,
            ldn, drop_mode, kp, ldkp, p, self.seed, self.offset, cw.data_ptr(), cb_.data_ptr(), m.emb_layer.weight.data_ptr(),
            m.emb_layer.bias.data_ptr(), self.E, B, self.I, bufs.xin.data_ptr(), bufs.xin.stride(0), bufs.xt.data_ptr(),
            bufs.xt.stride(0), bufs.temb.data_ptr(), _lib.stream_ptr()))
        bufs.xin_ones = True
        self._drop = (drop_mode, keep, p, self.offset, False)
        return x, noise, keep, xU

    def _cat_params(self):
        cw, cb_ = self.model.cat_layer.weight, self.model.cat_layer.bias
        _lib.require_gpu(cw, "DNNCat parameters")
        if not (cw.is_contiguous() and cb_.is_contiguous() and cw.dtype == torch.float32):
            raise RuntimeError("gdmcf_amd: DNNCat parameters must be contiguous float32")
        return cw, cb_

    def _train_input(self, bufs, spec, xt_out):
        x0 = core._f32_rows(spec["x_start"])
        xU = self._xU(bufs, x0.shape[0], x0.device)
        _, s8 = self.onehot_rows(x0, spec["ts_U"], spec["sampled"], spec["discrete"], out=xU)
        return self._cat_input(bufs, x0, xU, spec["ts"], spec["ca"], spec["cb"], spec["noise"], spec["drop_mask"],
                               self.model.training) + (s8,)

    def _train_input_csr(self, bufs, spec):
        """gdmcf_cat_prep_input_csr_f32 on spec["csr"] (data_utils.CsrBatch): bufs.xin and bufs.xt as _train_input leaves them,
        the rows in bufs.x0bits (the loss target), the classes in bufs.clsbits; no dense row, no one-hot image.  The Philox
        position advances as on the dense route (class draws, then the builder), so both routes draw the same numbers from the
        same seed."""
        batch, m = spec["csr"], self.model
        B, I = batch.shape
        if bufs.x0bits is None:
            bufs.x0bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=batch.device)
            bufs.clsbits = torch.zeros_like(bufs.x0bits)
        s8, ts_U, sampled = None, spec["ts_U"], spec["sampled"]
        if sampled is not None:
            s8 = (sampled if sampled.dtype == torch.uint8 else (sampled != 0).to(torch.uint8)).contiguous()
        elif ts_U is not None:
            ts_U = ts_U.to(device=batch.device, dtype=torch.int64).contiguous()
        self._cat_params()
        p = float(m.drop.p)
        self.offset += 2
        _, noise, keep, drop_mode = core.cat_prep_input_csr(
            self.lib, batch, ts_U, spec["discrete"], s8, self.seed, self.offset - 1, spec["ts"], spec["ca"], spec["cb"],
            spec["noise"], spec["drop_mask"], p, m.training, self.offset, m.cat_layer, m.emb_layer, self.E, bufs.xin, bufs.xt,
            bufs.temb, bufs.x0bits, bufs.clsbits, _lib.stream_ptr())
        bufs.xin_ones = True
        self._drop = (drop_mode, keep, p, self.offset, True)
        return None, noise, keep, batch, s8, ts_U

    # -- backward: the plain chain, then the cat layer ---------------------------------------------------------------------
    def _backward(self, sv, dz_last, rowscale):
        """Gradients in model.parameters() order: emb_layer (w, b), cat_layer (w, b), in_layers..., out_layers..."""
        if self.fused_opt is not None or self.grad_sink is not None:
            raise NotImplementedError("gdmcf_amd.DNNCat: no optimiser inside the backward pass and no gradient sink (the "
                                      "input gradient of the first layer reads its weight)")
        out = super()._backward(sv, dz_last, rowscale)
        bufs, layers, B = sv["bufs"], sv["layers"], sv["B"]
        m, st = self.model, _lib.stream_ptr()
        w1 = layers[0][0]
        # dxin = dZ1 . W1[:, 0:I]: bufs.dzs[0] is still d(loss)/d(first pre-activation), W1 is not updated before step()
        core.linear_bwd_input(self.lib, bufs, bufs.dzs[0], w1, None, None, 0, B, w1.shape[0], self.I, bufs.dxin, st)
        gw, gb = self._grad_like(m.cat_layer.weight), self._grad_like(m.cat_layer.bias)
        drop_mode, keep, p, offset, sparse = self._drop
        if sparse:  # the one-hot pair from the bitmaps the CSR-fed builder wrote
            core.cat_grad_bits(self.lib, bufs.dxin, bufs.xt, bufs.x0bits, bufs.clsbits, drop_mode, keep, p, self.seed, offset, B,
                               self.I, bufs.cat_ws, bufs.cat_ws_bytes, gw, gb, st)
            return out[:2] + [gw, gb] + out[2:]
        (kp, ldkp) = core._pl(keep)
        _lib.check(self.lib.gdmcf_cat_grad_f32(
            bufs.dxin.data_ptr(), bufs.dxin.stride(0), bufs.xt.data_ptr(), bufs.xt.stride(0), bufs.xU.data_ptr(),
            bufs.xU.stride(0), drop_mode, kp, ldkp, p, self.seed, offset, B, self.I, bufs.cat_ws.data_ptr(), bufs.cat_ws_bytes,
            gw.data_ptr(), gb.data_ptr(), st))
        return out[:2] + [gw, gb] + out[2:]

    # -- plain forward (evaluation / reverse loop) --------------------------------------------------------------------------
    @with_precision
    def forward_plain(self, x, timesteps, x_U, training, drop_mask=None, posterior=None):
        self.flush_weight_waiters()
        B, dev = x.shape[0], x.device
        layers = self._layers()
        bufs = self.buffers(B, dev)
        self._shadows_on(bufs, layers)
        self.version += 1
        self._saved = None
        ts = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        xu = x_U.reshape(B, -1)
        if xu.shape[1] != 2 * self.I:
            raise RuntimeError("gdmcf_amd.DNNCat: x_U must hold two columns per item")
        xu = core._f32_rows(xu)
        keep = self._cat_input(bufs, x, xu, ts, None, None, None, drop_mask, training)
        A = self._hidden_forward(bufs, layers, B)
        w, bias, act = layers[-1]
        res = self._last_layer(bufs, A, w, bias, act, B, w.shape[0], w.shape[1], keep[0], posterior)
        del keep
        return res

    # -- reverse loop in the first hidden layer's space (GaussianDiffusionDiscrete.p_sample(latent="extended")) ----------------
    def _latent_cat_tables(self, bufs, ops, B, sparse):
        """What the loop needs of cat_layer's parameters, which live on the device: per-row coefficient vectors [B] for
        gdmcf_latent_acc_f32 and, on CSR rows, the time table with (w1 + c) S added.  Made by torch from the parameters (no host
        read, no synchronisation) and kept until one of them or the operands change; the step table c1 . w0 [T, B] joins it in
        latent_loop (c1_src, c1)."""
        cw, cb_ = self._cat_params()
        key = (cw.data_ptr(), cw._version, cb_.data_ptr(), cb_._version, sparse)
        t = getattr(bufs, "lat_cat", None)
        if t is not None and t.key == key and t.ops is ops:
            return t
        wv, h = cw.detach().reshape(-1), ops.S.shape[0]
        t = _Bufs()
        t.key, t.ops, t.c1_src = key, ops, None
        t.w0 = wv[0].expand(B).contiguous()
        t.neg_w0 = -t.w0
        t.beta = (wv[2] - wv[1]).expand(B).contiguous()
        t.one, t.zero = torch.ones_like(t.w0), torch.zeros_like(t.w0)
        t.e = ops.e
        if sparse:
            t.e = ops.e.clone()
            t.e[:, :h] += (wv[1] + cb_.detach().reshape(-1)[0]) * ops.S
        bufs.lat_cat = t
        return t

    @with_precision
    def latent_loop(self, x_T, x_U, T, tabs32, index=None, before_step=None, stop=False, eps=None):
        """OneHotEngine.latent_loop's call for this backbone.  x_tU is the same image at every step and dropout is off, so the
        first layer's input is z_t = w0 x_t + u with u = w1 xU0 + w2 xU1 + c fixed, and its pre-activation is
            w0 p_t + r + e_t,    p_t = W1x x_t,   r = W1x u  [B, h], once per call.
        p~_t = w0 p_t is carried: the step of EngineBase._latent_reverse with c1 times w0 and the row addend r.
          x_T a data_utils.CsrBatch of binary rows (x_U None: xU0 = 1 - x, xU1 = x): r = (w1 + c) S + (w2 - w1) p_T with
            S = W1x 1 cached beside M and v; the first term is added to the time table, p_T is the one gather -- no [B, 2I]
            image, no builder.  Item-wide work: the last product.
          dense rows with the [B, 2I] image x_U: gdmcf_cat_prep_input_f32 once for z_T and x_T, two first-layer products
            (W1x z_T, W1x x_T), r = W1x z_T - w0 p_T.  Item-wide work: those two and the last product, whatever T is.
        eps / stop: as OneHotEngine.latent_loop.  The Philox position advances as on the item-space route (the class draws,
        then one builder per step), whether or not those kernels ran."""
        from .data_utils import CsrBatch
        self.flush_weight_waiters()
        lib, st, I = self.lib, _lib.stream_ptr(), self.I
        B, dev = x_T.shape[0], x_T.device
        layers = self._layers()
        bufs = self.buffers(B, dev)
        self._shadows_on(bufs, layers)
        self.version += 1
        self._saved = None
        w1 = layers[0][0]
        h1 = w1.shape[0]
        ops, tabs, p, ld = self._latent_begin(bufs, layers, T, B, tabs32)
        sparse = isinstance(x_T, CsrBatch)
        t = self._latent_cat_tables(bufs, ops, B, sparse)
        if getattr(bufs, "lat_pT", None) is None:
            bufs.lat_pT, bufs.lat_r, bufs.lat_s = (torch.zeros(B, ld, dtype=torch.float32, device=dev) for _ in range(3))
        pT, r, s = bufs.lat_pT, bufs.lat_r, bufs.lat_s
        if sparse:
            self.offset += 1 + T  # (the class draws and the T builders of the item-space route)
            keep = None
            core.gather_fwd(lib, None, None, x_T, self._transposed(w1), I, None, None, 0, None, 0, B, h1, pT, st)
            core.latent_acc(lib, r, t.zero, pT, t.beta, B, h1, r, st)  # r = (w2 - w1) p_T; (w1 + c) S sits in t.e
            xdense = None if stop else x_T.dense()
        else:
            xu = x_U.reshape(B, -1)
            if xu.shape[1] != 2 * I:
                raise RuntimeError("gdmcf_amd.DNNCat: x_U must hold two columns per item")
            ts = torch.full((B,), T - 1, dtype=torch.int64, device=dev)
            keep = self._cat_input(bufs, x_T, core._f32_rows(xu), ts, None, None, None, None, False), ts  # xin = z_T, xt = x_T
            self.offset += T - 1
            core.linear_fwd(lib, bufs, (bufs.xin.data_ptr(), bufs.xin.stride(0)), w1, None, 0, B, h1, I, s, st)
            core.linear_fwd(lib, bufs, (bufs.xt.data_ptr(), bufs.xt.stride(0)), w1, None, 0, B, h1, I, pT, st)
            core.latent_acc(lib, s, t.one, pT, t.neg_w0, B, h1, r, st)  # r = W1x z_T - w0 p_T
            xdense = bufs.xt
        core.latent_acc(lib, p, t.zero, pT, t.w0, B, h1, p, st)  # p~_T = w0 p_T
        core.latent_acc(lib, p, t.one, r, t.one, B, h1, s, st)  # p~_T + r: the first activation's pre-activation without e

        def c1_of(c1):  # the step table c1 . w0 [T, B], kept while `t` and the table stay
            if t.c1_src is not c1:
                t.c1_src, t.c1 = c1, c1 * t.w0[0]
            return t.c1

        x0 = self._latent_run(bufs, layers, ops, tabs, T, B, s, p, t.e, xdense, stop=stop, eps=eps, r=r, c1_of=c1_of,
                              before_step=before_step)
        del keep
        return x0


class DNNCat(nn.Module):
    """Drop-in for the reference DNNCat (models/DNN.py:180-265)."""

    # the latent loop under latent="extended" only; CSR rows on that route only, without a second-branch handle (xU0 = 1 - x, xU1 = x)
    reverse_carries = Carries("extended", False, sparse_latent=True, second_handle=False)
    csr_rows = False  # training_losses densifies a CsrBatch for this backbone unless the instance was built with csr_rows=True
    fused_update_refusal = ("the input gradient of the first layer reads its weight, which a fused update would overwrite "
                            "first; use the separate AdamW pass")

    def __init__(self, in_dims, out_dims, emb_size, time_type="cat", norm=False, dropout=0.5, cat_dim=2, gemm_dtype="f32",
                 csr_rows=False):
        """csr_rows=True: a data_utils.CsrBatch handed to training_losses stays sparse (module docstring); the default
        densifies it."""
        super().__init__()
        if norm:
            raise NotImplementedError("gdmcf_amd.DNNCat: norm=True needs a row norm between the mix and the dropout")
        if gemm_dtype != "f32":
            raise NotImplementedError("gdmcf_amd.DNNCat: GEMM inputs other than f32 (%s) are not built" % gemm_dtype)
        if cat_dim != 2:
            raise NotImplementedError("gdmcf_amd.DNNCat: the input kernel mixes x_t with one-hot PAIRS (cat_dim = 2)")
        self.gemm_dtype = gemm_dtype
        if csr_rows:
            self.csr_rows = True  # (on the instance only: the class attribute is the default)
        self.in_dims = list(in_dims)
        self.out_dims = list(out_dims)
        assert out_dims[0] == in_dims[-1], "In and out dimensions must equal to each other."
        self.time_type = time_type
        self.time_emb_dim = emb_size
        self.norm = norm
        self.emb_layer = nn.Linear(self.time_emb_dim, self.time_emb_dim)
        self.cat_layer = nn.Linear(cat_dim + 1, 1)  # torch's default nn.Linear init, as in the reference
        if self.time_type == "cat":
            in_dims_temp = [self.in_dims[0] + self.time_emb_dim] + self.in_dims[1:]
        else:
            raise ValueError("Unimplemented timestep embedding type %s" % self.time_type)
        out_dims_temp = self.out_dims
        self.in_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(in_dims_temp[:-1], in_dims_temp[1:])])
        self.out_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(out_dims_temp[:-1], out_dims_temp[1:])])
        self.drop = nn.Dropout(dropout)  # holds p; the mask is applied inside the HIP input kernel
        self.init_weights()
        self._engine = None

    def init_weights(self):
        for layer in list(self.in_layers) + list(self.out_layers) + [self.emb_layer]:
            fan_out, fan_in = layer.weight.size()
            layer.weight.data.normal_(0.0, np.sqrt(2.0 / (fan_in + fan_out)))
            layer.bias.data.normal_(0.0, 0.001)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = CatEngine(self)
        return self._engine

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None
        return state

    def layer_list(self):
        """[(weight, bias, act)] of the dense layers behind the cat layer; act 1 = tanh, 0 = none (reference :256-263)."""
        layers = [(l.weight, l.bias, 1) for l in self.in_layers]
        n_out = len(self.out_layers)
        layers += [(l.weight, l.bias, 1 if i != n_out - 1 else 0) for i, l in enumerate(self.out_layers)]
        return layers

    def param_list(self):
        return list(self.parameters())

    def forward(self, x, timesteps, x_U, drop_mask=None, posterior=None):
        """model(x_t, t, x_tU) of the reference's evaluation path; x_U is [B, I, 2] or [B, 2I].  Training goes through
        GaussianDiffusionDiscrete.training_losses (fused forward + loss with its own backward); this plain forward carries
        no autograd graph.  `posterior` (reverse loop, see OneHotEngine._last_layer): return (x_{t-1}, pred_xstart) with the
        posterior mean fused into the output GEMM instead of the raw output."""
        _lib.require_gpu(x, "DNNCat input")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and self.training:
            raise RuntimeError("gdmcf_amd.DNNCat: the plain forward is not differentiable; train through "
                               "GaussianDiffusionDiscrete.training_losses (or call under torch.no_grad())")
        return self.engine.forward_plain(x, timesteps, x_U, self.training, drop_mask, posterior=posterior)
