"""Drives the C ABI (include/gdmcf_hip.h) for one DNN denoiser: owns the HBM workspaces and the
order of kernel launches for
  * the fused training forward  (q_sample -> dropout -> layers -> row loss -> f64 tail)
  * its backward                (weight / bias / embedding gradients)
  * the plain forward/backward  (model(x, t))
  * the reverse-diffusion loop  (p_sample).
PyTorch is used for device memory and streams only; every arithmetic step is a HIP kernel.

HBM layout (all float32 row-major, leading dims padded to 64 elements = 256 B):
  xin   [B, ldk]  first-layer input  [ drop(x_t) | emb(t) | 0-pad ],  ldk = ceil64(I + E)
  act_l [B, ld_l] tanh outputs of every layer but the last
  diff  [B, ldi]  alpha*out - target (the last layer's output is never stored in training)
  slabs           split-K partial sums (forward of layer 0, input-gradient of the last layer)
"""

import ctypes
import os

import torch

from . import _lib
from . import engine_core as core
from .engine_core import EngineBase, _Bufs, _ceil64, with_precision


class DenoiserEngine(EngineBase):
    def __init__(self, model):
        super().__init__(model)
        self._wshadow = {}
        # compute a layer's input gradient before its weight gradient (needed when the weight may be updated as
        # soon as its gradient exists: fused optimiser, single-process early update in parallel.DataParallelStep)
        self.input_grad_first = False
        # id(weight) -> callable that makes the current stream wait until the weight is complete.  Set by the sharded
        # data-parallel optimiser, whose all-gather of the other ranks' updated rows may still be on the wire when the
        # next step starts: train_forward waits per layer, right before the first GEMM that reads the weight, so the
        # last layer's gather travels under the first layers' GEMMs.  Every other entry point waits for all up front.
        self.weight_waiters = {}
        # gradients in persistent buffers (one per parameter, reused every step) instead of fresh tensors: constant
        # addresses for a step captured in a hipGraph (gdmcf_amd/graph.py); a `.grad` kept across steps is overwritten
        self.static_grads = False
        self._grad_bufs = {}
        # opt-in (GDMCF_GEMM_SIDE=1), single GPU: the last layer's weight-gradient GEMM on a second stream beside the
        # input-gradient GEMM (both only read dZ; each fills the other's partial last round of workgroups).  Measured
        # 1.692 -> 1.673 ms per Yelp-shape step, 4.276 -> 4.251 ms at the Amazon-Book shape, bit-identical results.  Off by
        # default: two GEMMs sharing the chip cannot be timed one by one (HIP events / rocprof show 0.44 + 0.35 ms for the
        # pair instead of 0.26 + 0.23), and the per-kernel roofline is what bench.py reports.
        self._gemm_side = os.environ.get("GDMCF_GEMM_SIDE", "0") == "1"
        self._side2 = None
        self._side2_used = False
        self._wt_on = os.environ.get("GDMCF_FWD_WT", "1") == "1"
        # Deferred loss tail.  A caller that runs train_backward(1 / B) right behind training_losses
        # (parallel.DataParallelStep's direct backward, and GraphedTrainStep through it) sets `defer_tail` around that call:
        # train_forward then launches neither the loss tail nor the last layer's row scale, and the backward's FIRST launch --
        # gdmcf_linear_bwd_input_tail_f32, the last layer's input gradient -- carries them on a workgroup the product leaves idle.
        # Until then losses["loss"], last_loss_mean, bufs.rowscale_mean / gradcoef / lu / hs and the Lt history of that step are
        # UNWRITTEN; anything else that follows a deferred forward runs the tail on its own first (_flush_tail).
        self.defer_tail = False
        self._pending_tail = None

    def _grad_like(self, p):
        if not self.static_grads:
            return torch.empty_like(p)
        g = self._grad_bufs.get(id(p))
        if g is None or g.shape != p.shape or g.device != p.device:
            g = self._grad_bufs[id(p)] = torch.empty_like(p)
        return g

    def _use_weight(self, w):
        fn = self.weight_waiters.pop(id(w), None) if self.weight_waiters else None
        if fn is not None:
            fn()
            rec = self._wshadow.get(id(w))
            if rec is not None and rec[1] != w._version:
                rec[0].sync()
                rec[1] = w._version

    def flush_weight_waiters(self):
        self._flush_tail()
        while self.weight_waiters:
            self.weight_waiters.popitem()[1]()

    def _defers_tail(self, spec, layers, B):
        """Whether this training forward leaves its loss tail to the backward: asked for (defer_tail), the plain DNN engine, float32
        products, x0 target, no data-parallel gradient sink, and a last layer whose input gradient the register-streaming kernel takes with a
        workgroup to spare."""
        if not self.defer_tail or type(self) is not DenoiserEngine or self.gemm_dtype != "f32" or spec["eps_mode"]:
            return False
        if (self.grad_sink is not None and not self.input_grad_first) or len(layers) < 2:  # (a data-parallel sink wants dW first)
            return False
        n, k = layers[-1][0].shape
        return bool(self.lib.gdmcf_debug_kn_tail_rides(B, k, n))

    def _flush_tail(self):
        """Runs the tail of a deferred training forward whose backward has not come, as launches of its own: no tensor of that
        step stays unwritten."""
        pend, self._pending_tail = self._pending_tail, None
        if pend is not None:
            core.tail_job_run(self.lib, pend[0], pend[1], _lib.stream_ptr())

    # ------------------------------------------------------------------------------------------
    # bf16 shadows (gemm_dtype == "bf16"): bf16 copies of every GEMM operand, streamed instead of the f32 tensors.
    # Activation shadows are written by the kernels that produce the activations; weight shadows are refreshed
    # here whenever the parameter's version counter moved (FusedAdamW bumps it after its raw-pointer update).
    def _shadows_on(self, bufs, layers):
        if self.gemm_dtype != "bf16":
            if bufs.shadows is not None:  # precision switched back: drop the registrations
                for sh in bufs.shadows:
                    sh.close()
                bufs.shadows = None
                bufs.sh_xin2 = None
            for sh, _ in self._wshadow.values():
                sh.close()
            self._wshadow = {}
            return
        if bufs.shadows is None:
            I, E = self.I, self.E
            mk = lambda t, cols: _lib.Bf16Shadow(t[:, :cols], sync=False)
            sh = [mk(bufs.xin, I + E), mk(bufs.diff, I)]
            for (w, _, _), a, d in zip(layers[:-1], bufs.acts, bufs.dzs):
                sh += [mk(a, w.shape[0]), mk(d, w.shape[0])]
            sh.append(mk(bufs.hs, layers[-1][0].shape[1]))
            bufs.shadows = sh
            bufs.sh_xin = sh[0]
        live = {id(w) for w, _, _ in layers}
        for key in [k for k in self._wshadow if k not in live]:  # a parameter object was replaced: drop its registration
            self._wshadow.pop(key)[0].close()
        for w, _, _ in layers:
            rec = self._wshadow.get(id(w))
            if rec is None or rec[0].ptr != w.data_ptr():
                self._use_weight(w)  # the first cast reads the weight
                if rec is not None:
                    rec[0].close()
                self._wshadow[id(w)] = [_lib.Bf16Shadow(w.detach()), w._version]
            elif id(w) in self.weight_waiters:
                continue  # still arriving: refreshed in _use_weight
            elif rec[1] != w._version:
                rec[0].sync()
                rec[1] = w._version

    def _layers(self):
        layers = self.model.layer_list()
        self._check_params(layers)
        return layers

    def buffers(self, B, device):
        key = (B, str(device))
        b = self._bufs.get(key)
        if b is not None:
            return b
        layers = self.model.layer_list()
        f32 = dict(dtype=torch.float32, device=device)
        b = _Bufs()
        b.ldk = _ceil64(self.I + self.E)
        b.xin = torch.zeros(B, b.ldk, **f32)
        b.xin2 = None
        b.acts = [torch.zeros(B, _ceil64(w.shape[0]), **f32) for (w, _, _) in layers[:-1]]
        b.dzs = [torch.zeros(B, _ceil64(w.shape[0]), **f32) for (w, _, _) in layers[:-1]]
        b.hs = torch.zeros(B, _ceil64(layers[-1][0].shape[1]), **f32)
        b.shadows = None  # bf16 shadows of the GEMM operands among these buffers (created on first bf16 use)
        self._shared_buffers(b, B, device, layers[-1][0].shape[0], layers[0][0].shape[0], [w for w, _, _ in layers])
        self._bufs[key] = b
        return b

    # ------------------------------------------------------------------------------------------
    def _prep(self, bufs, x, ts, ca, cb, noise, drop_mask, training, xt_out=None, xin=None):
        xin = bufs.xin if xin is None else xin
        keepalive = self._prep_input(bufs, x, self.I, xin, ts, ca, cb, noise, drop_mask, training, xt_out=xt_out)
        if xin is bufs.xin:
            bufs.xin_ones = True  # (the builder leaves 1 in column I + E: the bias column of the first layer's weight gradient)
        return keepalive

    def _train_input(self, bufs, spec, xt_out):
        """The first layer's input of a training step on dense rows (a backbone with its own input step overrides this);
        returns (x0, noise, ...) as the kernels read them, to keep referenced."""
        return self._prep(bufs, spec["x_start"], spec["ts"], spec["ca"], spec["cb"], spec["noise"], spec["drop_mask"],
                          self.model.training, xt_out=xt_out)

    def _prep_csr(self, bufs, batch, ts, ca, cb, noise, drop_mask, training):
        """First-layer input straight from the device CSR rows of `batch` (data_utils.CsrBatch): no dense x0 anywhere; the
        rows' bitmaps go to bufs.x0bits for the loss epilogue."""
        m = self.model
        B, I = batch.shape
        if getattr(bufs, "x0bits", None) is None:
            bufs.x0bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=batch.device)
        self.offset += 1
        keepalive = core.prep_input_csr(self.lib, batch, ts, ca, cb, noise, drop_mask, float(m.drop.p), training, self.seed,
                                        self.offset, m.emb_layer, self.E, bufs.xin, bufs.temb, bufs.x0bits, _lib.stream_ptr())
        bufs.xin_ones = True
        return keepalive

    def _train_input_csr(self, bufs, spec):
        """The first layer's input of a training step on rows that stay sparse (spec["csr"]; a backbone with its own input step
        overrides this); returns (None or x0, noise, ...) to keep referenced -- the x0 target is bufs.x0bits."""
        return self._prep_csr(bufs, spec["csr"], spec["ts"], spec["ca"], spec["cb"], spec["noise"], spec["drop_mask"],
                              self.model.training)

    def _hidden_forward(self, bufs, layers, B, xin=None, frozen=False, csr=None):
        """All layers but the last; returns the activation feeding the last layer.  frozen: the caller runs many forward passes over
        unchanged weights (reverse loop): large layers go through their cached transposes.  csr: the first-layer input holds the
        binary, undropped rows of this data_utils.CsrBatch (first reverse step from x_0): the first layer is a gather of nnz rows of
        its cached transpose instead of a product."""
        lib, st = self.lib, _lib.stream_ptr()
        A = bufs.xin if xin is None else xin
        for li, (w, bias, act) in enumerate(layers[:-1]):
            N, K = w.shape
            out = bufs.acts[li]
            self._use_weight(w)
            if li == 0 and csr is not None:
                self._gather_first_layer(bufs, csr, w, bias, act, A, B, out, st)
            elif frozen and self._wt_on and self.gemm_dtype == "f32" and K >= 4096 and w.numel() >= (1 << 20):
                wt = self._transposed(w)
                _lib.check(lib.gdmcf_linear_fwd_wt_f32(A.data_ptr(), A.stride(0), wt.data_ptr(), wt.stride(0), bias.data_ptr(), act, B, N, K,
                                                       out.data_ptr(), out.stride(0), bufs.ws.data_ptr(), bufs.ws_bytes, st))
            else:
                core.linear_fwd(lib, bufs, A, w, bias, act, B, N, K, out, st)
            A = out
        return A

    # ------------------------------------------------------------------------------------------
    # fused training forward / backward
    # ------------------------------------------------------------------------------------------
    @with_precision
    def train_forward(self, spec):
        """loss [B] (float64).  With `defer_tail` set and _defers_tail true, the returned tensor and last_loss_mean are written by
        the FIRST launch of the train_backward(1 / B) that follows (see __init__)."""
        self._flush_tail()
        x0, ts = spec["x_start"], spec["ts"]
        csr = spec.get("csr")
        B, dev = (csr.shape[0], csr.device) if csr is not None else (x0.shape[0], x0.device)
        layers = self._layers()
        bufs = self.buffers(B, dev)
        self._shadows_on(bufs, layers)
        lib, st = self.lib, _lib.stream_ptr()
        self.version += 1
        eps_mode = spec["eps_mode"]
        xt_out = None
        if eps_mode:
            if bufs.xt is None:
                bufs.xt = torch.zeros(B, bufs.ldi, dtype=torch.float32, device=dev)
            xt_out = bufs.xt
        if csr is not None:
            keepalive = self._train_input_csr(bufs, spec)
        else:
            keepalive = self._train_input(bufs, spec, xt_out)
        x0c = keepalive[0]
        alpha = None
        if eps_mode:
            # target = eps, except rows with t == 0 whose term is the x0-likelihood
            # mean((x0 - (r1*x_t - r2*eps_hat))^2 / 2)  (reference gaussian_diffusion.py:344-348)
            target, alpha, rowdiv = self._eps_target(bufs, spec, ts, x0c, keepalive[1])
        else:
            target = x0c
            rowdiv = bufs.rowdiv_mse
        A = self._hidden_forward(bufs, layers, B)
        w, bias, _ = layers[-1]
        N, K = w.shape
        self._use_weight(w)
        defer = self._defers_tail(spec, layers, B)
        if csr is not None:  # the target rows are bitmaps written by the CSR-fed input builder
            nt = core.loss_layer_bits(lib, bufs, A, w, bias, bufs.x0bits, None, B, N, K, st, reduce=not defer)
        else:
            nt = core.loss_layer(lib, bufs, A, w, bias, target, alpha, B, N, K, st, reduce=not defer)
        # the tail also emits mean(loss) and gradcoef/B: the reference's step takes the mean next (main.py:348), and its
        # backward scales every row by 1/B -- two launches less per step (DataParallelStep uses both)
        tail = None
        if defer:  # row-partial reduction, tail and the last layer's row scale: in the backward's first launch
            loss, self.last_loss_mean, tail = core.loss_tail_job(lib, bufs, spec, B, rowdiv, alpha, nt, A, K)
            self._pending_tail = (tail, B)
        else:
            loss, self.last_loss_mean = core.loss_tail(lib, bufs, spec, B, rowdiv, alpha, st, mean=True)
        self._saved = dict(kind="train", B=B, bufs=bufs, layers=layers, tail=tail,
                           keepalive=(keepalive, target, alpha, rowdiv, spec["pt"]))
        return loss

    @with_precision
    def train_backward(self, gloss):
        """gloss: d(total)/d(loss_b) as a tensor [B] (what autograd hands over), or a Python float when every row has
        the same upstream gradient (mean reduction: 1/B) -- then no autograd graph is needed at all."""
        sv = self._saved
        if sv is None or sv.get("kind") != "train":
            raise RuntimeError("gdmcf_amd: train_backward without a preceding training_losses")
        bufs = sv["bufs"]
        tail = sv.get("tail")
        if tail is not None and self._pending_tail is not None and self._pending_tail[0] is tail:
            if isinstance(gloss, float) and gloss == 1.0 / sv["B"]:
                # the deferred tail rides the last layer's input gradient, which reads the row scale it writes only behind a
                # kernel boundary (the split-K reducer)
                self._pending_tail = None
                return self._backward(sv, bufs.diff, bufs.rowscale_mean, tail=tail)
            self._flush_tail()
        if isinstance(gloss, float) and gloss == 1.0 / sv["B"] and getattr(bufs, "rowscale_mean", None) is not None:
            rowscale = bufs.rowscale_mean  # gradcoef * (float)(1/B), written by the loss tail: same bits as the product below
        else:
            rowscale = self._rowscale_of(bufs, gloss)
        return self._backward(sv, bufs.diff, rowscale)

    # ------------------------------------------------------------------------------------------
    # plain forward / backward (model(x, t))
    # ------------------------------------------------------------------------------------------
    @with_precision
    def forward_plain(self, x, timesteps, training, drop_mask=None):
        self.flush_weight_waiters()
        B, dev = x.shape[0], x.device
        layers = self._layers()
        bufs = self.buffers(B, dev)
        self._shadows_on(bufs, layers)
        lib, st = self.lib, _lib.stream_ptr()
        self.version += 1
        ts = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        keepalive = self._prep(bufs, x, ts, None, None, None, drop_mask, training)
        A = self._hidden_forward(bufs, layers, B)
        w, bias, act = layers[-1]
        N, K = w.shape
        out = torch.empty(B, N, dtype=torch.float32, device=dev)
        core.linear_fwd(lib, bufs, A, w, bias, act, B, N, K, out, st)
        self._saved = dict(kind="plain", B=B, bufs=bufs, layers=layers, keepalive=(keepalive, ts))
        return out

    @with_precision
    def backward_plain(self, gout):
        sv = self._saved
        g = gout.to(torch.float32)
        if g.stride(-1) != 1:
            g = g.contiguous()
        return self._backward(sv, g, None)

    # ------------------------------------------------------------------------------------------
    def _backward(self, sv, dz_last, rowscale, tail=None):
        """Gradients in model.parameters() order: emb_layer (w, b), in_layers..., out_layers...
        dz_last is d(loss)/d(last layer output) up to the per-row factor `rowscale`.
        tail: the job of a deferred training forward (engine_core.loss_tail_job).  The last layer's input gradient then comes first
        and carries it (gdmcf_linear_bwd_input_tail_f32): that launch writes `rowscale` and the row-scaled copy bufs.hs, which
        the last layer's weight gradient reads without a row-scale launch of its own.

        Order inside a layer: data parallel wants the weight gradient first (its all-reduce then overlaps the
        input-gradient GEMM); the fused optimiser needs the input gradient first (it reads W, which the
        weight-gradient epilogue then overwrites)."""
        lib, st = self.lib, _lib.stream_ptr()
        bufs, layers, B = sv["bufs"], sv["layers"], sv["B"]
        m = self.model
        L = len(layers)
        grads_w = [None] * L
        grads_b = [None] * L
        dWe = dbe = None
        fused = self.fused_opt if self.grad_sink is None else None
        dz, rs = dz_last, rowscale
        # f32 products of fused weights: queued and issued as ONE launch after every input gradient (one ramp, one optimiser-stream
        # drain and one ragged last round of tiles per step instead of one per weight).  Their operands -- the per-layer dzs, the
        # row-scaled copy bufs.hs (written for the last layer only) and the activations -- are not written again before that.
        # GDMCF_DW_MULTI=0: one launch per weight, where its layer's backward issues it.
        dw_queue = [] if (fused is not None and self.gemm_dtype == "f32" and os.environ.get("GDMCF_DW_MULTI", "1") != "0") else None

        def input_grad(li, w, A_prev):
            nonlocal dWe, dbe
            N, K = w.shape
            if li > 0:
                dprev = bufs.dzs[li - 1]
                if tail is not None and li == L - 1:
                    core.linear_bwd_input_tail(lib, bufs, dz, w, rs, A_prev, layers[li - 1][2], B, N, K, dprev, tail, st)
                else:
                    self._input_grad(bufs, B, w, N, K, dz, rs, A_prev, layers[li - 1][2], dprev, st)
                return dprev
            dWe = self._grad_like(m.emb_layer.weight)
            dbe = self._grad_like(m.emb_layer.bias)
            core.emb_bwd(lib, bufs, dz, w, self.I, self.E, B, N, dWe, dbe, st)
            return None

        def weight_grad(li, w, bias, A_prev):
            db = self._grad_like(bias)
            # without a row scale, the first layer's input already holds 1 in its first padding column (the input builder's)
            scol = int(rs is None and li == 0 and getattr(bufs, "xin_ones", False) and A_prev.stride(0) > w.shape[1])
            if tail is not None and li == L - 1:  # the tail job wrote bufs.hs, its column K included
                A_use, scol = bufs.hs, int(bufs.hs.stride(0) > w.shape[1])
            else:
                A_use, scol = self._row_scaled(bufs, B, w.shape[1], A_prev, rs, scol, st)
            fs = fused.fused_state(w) if fused is not None else None
            dW = self._grad_like(w) if fs is None else None
            if fs is None and self._gemm_side and self.grad_sink is None and li == L - 1 and L > 1:
                # the last layer's weight-gradient GEMM on a second stream, beside the input-gradient GEMM
                if self._side2 is None:
                    self._side2 = torch.cuda.Stream()
                self._side2.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(self._side2):
                    self._weight_grad(bufs, B, w, dz, rs, A_use, scol, dW, db, None, _lib.stream_ptr())
                self._side2_used = True
            else:
                self._weight_grad(bufs, B, w, dz, rs, A_use, scol, dW, db, fs, st, queue=dw_queue)
            grads_w[li], grads_b[li] = dW, db
            if self.grad_sink is not None:
                self.grad_sink(w, dW)
                self.grad_sink(bias, db)
                grads_w[li] = grads_b[li] = None

        for li in range(L - 1, -1, -1):
            w, bias, _ = layers[li]
            A_prev = bufs.acts[li - 1] if li > 0 else bufs.xin
            if fused is not None or self.input_grad_first or (tail is not None and li == L - 1):
                nxt = input_grad(li, w, A_prev)
                weight_grad(li, w, bias, A_prev)
            else:
                weight_grad(li, w, bias, A_prev)
                nxt = input_grad(li, w, A_prev)
            dz, rs = nxt, None
        if dw_queue:
            arr = (_lib.GdDwAdamw * len(dw_queue))(*[e for e, _ in dw_queue])
            _lib.check(lib.gdmcf_linear_bwd_weight_adamw_multi_f32(ctypes.addressof(arr), len(dw_queue), st))
            for _, w in dw_queue:
                torch.autograd.graph.increment_version(w)  # updated in the GEMM epilogue
        if self._side2_used:  # everything that consumes the gradients is ordered behind the side stream
            torch.cuda.current_stream().wait_stream(self._side2)
            self._side2_used = False
        if self.grad_sink is not None:
            self.grad_sink(m.emb_layer.weight, dWe)
            self.grad_sink(m.emb_layer.bias, dbe)
            dWe = dbe = None
        out = [dWe, dbe]
        for li in range(L):
            out += [grads_w[li], grads_b[li]]
        return out

    # ------------------------------------------------------------------------------------------
    # reverse diffusion loop (reference gaussian_diffusion.py:161-220)
    # ------------------------------------------------------------------------------------------
    @with_precision
    def p_sample_loop(self, x_start, steps, T, tabs32, eps_mode, sampling_noise, noise0=None, step_noise=None,
                      capture=None, draw_noise=None, latent=False, stop=False, eps=None):
        """latent: carry the loop in the first hidden layer's space (_latent_loop; the caller has checked
        GaussianDiffusion._latent_reverse_ok).  stop (with latent; gdmcf_amd.recommend): end the loop before its last product and
        return that product's engine_core.LatentProduct instead of x_0.  eps (with latent and eps_mode; p_sample(latent="extended")):
        the engine_core.EpsTables of the schedule -- the EPSILON target's latent loop.
        tabs32: dict of float32 device tables [T] (sqrt_ab, sqrt_1mab, c1, c2, r1, r2, sigma).  draw_noise(like) -> [B, I]
        float32 N(0,1): the reverse loop's th.randn_like(x_t) (reference :210-217); default: gdmcf_randn_f32 on the engine's
        Philox seed (stream 7, one offset per draw).
        x_start may be a data_utils.CsrBatch where GaussianDiffusion._sparse_reverse_ok holds (steps == 0, binary rows, no
        F.normalize, no dropout, float32 products): x_T = x_0 is written into the first-layer input by the CSR-fed builder (the
        posterior epilogue needs the dense x_t), and the first step's first hidden layer is a gather of the rows' few dozen
        weight rows (gdmcf_gather_fwd_f32) instead of the [B, I + E] x [I + E, N] product.  Steps T-2 .. 0 run as on dense rows."""
        m, lib = self.model, self.lib
        if draw_noise is None:
            def draw_noise(like):
                self.offset += 1
                return _lib.philox_randn(like.shape, like.device, self.seed, self.offset, 7)
        self.flush_weight_waiters()
        B, dev, I = x_start.shape[0], x_start.device, self.I
        from .data_utils import CsrBatch
        csr = x_start if isinstance(x_start, CsrBatch) else None
        if csr is not None and (steps != 0 or m.norm or self.gemm_dtype != "f32" or csr.csr.values is not None):
            raise RuntimeError("gdmcf_amd: the reverse loop takes CSR rows only for steps == 0, binary rows, norm=False and "
                               "float32 products (GaussianDiffusion.p_sample densifies the rest)")
        layers = self._layers()
        bufs = self.buffers(B, dev)
        self._shadows_on(bufs, layers)
        st = _lib.stream_ptr()
        self.version += 1
        if latent:
            if (eps_mode and eps is None) or sampling_noise or capture is not None or m.norm or self.gemm_dtype != "f32":
                raise RuntimeError("gdmcf_amd: the latent reverse loop takes the x0 target without sampling noise, capture or "
                                   "F.normalize, in float32 products (GaussianDiffusion._latent_reverse_ok)")
            return self._latent_loop(bufs, layers, x_start, csr, steps, T, tabs32, noise0, stop=stop, eps=eps if eps_mode else None)
        if bufs.xin2 is None:
            bufs.xin2 = torch.zeros_like(bufs.xin)
        if self.gemm_dtype == "bf16" and getattr(bufs, "sh_xin2", None) is None:
            bufs.sh_xin2 = _lib.Bf16Shadow(bufs.xin2[:, : I + self.E], sync=False)
            bufs.shadows.append(bufs.sh_xin2)
        norm = bool(m.norm)
        keep = []
        t_vec = torch.full((B,), max(steps - 1, 0), dtype=torch.int64, device=dev)
        ca = cb = None
        if steps > 0:
            ca, cb = tabs32["sqrt_ab"], tabs32["sqrt_1mab"]
        w, bias, _ = layers[-1]
        N, K = w.shape
        out = None

        # per-step coefficient vectors [B] and timestep vectors: expanded ONCE per (schedule, batch size) into [T, B]
        # tables whose rows are used as they stand (was 3-6 tiny launches per reverse step)
        stabs = core.step_tables(tabs32, T, B, ("c1", "c2", "r1", "r2", "sigma"), bufs.tab_cache)
        if getattr(bufs, "step_ts", None) is None or bufs.step_ts.shape[0] != T:
            bufs.step_ts = torch.arange(T, dtype=torch.int64, device=dev)[:, None].expand(T, B).contiguous()
        step_ts = bufs.step_ts

        def posterior(i, n, A, xt, xn):
            c1, c2 = stabs["c1"][i], stabs["c2"][i]
            r1 = r2 = sg = z = None
            if eps_mode:
                r1, r2 = stabs["r1"][i], stabs["r2"][i]
            if sampling_noise and i != 0:
                sg = stabs["sigma"][i]
                z = step_noise[n] if step_noise is not None else draw_noise(xt[:, :I])
                z = z.contiguous()
            pred = torch.empty(B, I, dtype=torch.float32, device=dev) if capture is not None else None
            core.posterior_fwd(lib, A, w, bias, xt, c1, c2, r1, r2, sg, z, B, N, K, xn, pred, st)
            keep.append((c1, c2, r1, r2, sg, z))
            if capture is not None:
                capture.setdefault("pred_xstart", []).append(pred)
                capture.setdefault("mean", []).append(xn[:, :I].clone())

        if not norm:
            # x_t lives in the first-layer input buffers themselves: the posterior epilogue of step i writes x_{t-1}
            # straight into the other buffer's first I columns, a tiny kernel adds that step's embedding columns
            # (no per-step input builder: 2 x 55 MB less traffic per step at Yelp shape).
            cur, nxt = bufs.xin, bufs.xin2
            if csr is not None:
                keep.append(self._prep_csr(bufs, csr, t_vec, None, None, None, None, False))  # x_T = x_0, into bufs.xin
            else:
                keep.append(self._prep(bufs, x_start, t_vec, ca, cb, noise0, None, False, xin=cur))  # x_T
            bufs.xin_ones = False  # (gdmcf_dnn_emb_cols_f32 below rewrites the padding columns with zeros)
            for n, i in enumerate(range(T - 1, -1, -1)):
                ts = step_ts[i]
                _lib.check(lib.gdmcf_dnn_emb_cols_f32(ts.data_ptr(), m.emb_layer.weight.data_ptr(),
                                                      m.emb_layer.bias.data_ptr(), self.E, B, I, cur.data_ptr(),
                                                      cur.stride(0), bufs.temb.data_ptr(), st))
                keep.append(ts)
                A = self._hidden_forward(bufs, layers, B, xin=cur, frozen=True, csr=csr if n == 0 else None)
                out = torch.empty(B, I, dtype=torch.float32, device=dev) if i == 0 else None
                posterior(i, n, A, cur, out if out is not None else nxt)
                cur, nxt = nxt, cur
        else:
            # F.normalize needs the row norms of every x_t: keep x_t separate and rebuild the layer input per step
            if bufs.xt is None:
                bufs.xt = torch.zeros(B, bufs.ldi, dtype=torch.float32, device=dev)
            xt = bufs.xt
            keep.append(self._prep(bufs, x_start, t_vec, ca, cb, noise0, None, False, xt_out=xt, xin=bufs.xin2))
            for n, i in enumerate(range(T - 1, -1, -1)):
                ts = step_ts[i]
                keep.append(self._prep(bufs, xt[:, :I], ts, None, None, None, None, False, xin=bufs.xin))
                A = self._hidden_forward(bufs, layers, B, xin=bufs.xin, frozen=True)
                out = torch.empty(B, I, dtype=torch.float32, device=dev) if i == 0 else None
                xn = out if out is not None else (bufs.diff if xt is bufs.xt else bufs.xt)
                posterior(i, n, A, xt, xn)
                xt = xn
        self._saved = None
        del keep
        return out

    def _latent_begin(self, bufs, layers, T, B, tabs32):
        """What a latent loop of this layer chain starts from, every weight waited for: (cached operands, [T, B] c1 / c2, p and
        its row width)."""
        for wl, _, _ in layers:
            self._use_weight(wl)
        (w1, b1, _), (w, bias, _), emb = layers[0], layers[-1], self.model.emb_layer
        ops = self._latent_operands(w1, b1, w, w.shape[1], bias, T, (w1, b1, w, bias, emb.weight, emb.bias))
        ld = _ceil64(w1.shape[0])
        if getattr(bufs, "lat_p", None) is None:
            bufs.lat_p = torch.zeros(B, ld, dtype=torch.float32, device=w1.device)
            bufs.lat_h = torch.zeros_like(bufs.lat_p)
        return ops, core.step_tables(tabs32, T, B, ("c1", "c2"), bufs.tab_cache), bufs.lat_p, ld

    def _latent_run(self, bufs, layers, ops, tabs, T, B, pre, p, e, x_T, **kw):
        """EngineBase._latent_reverse on this layer chain: the first activation alternates between two buffers (with one hidden
        layer it is the step kernel's operand A as well), the layers between it and the last product are the small ones."""
        (_, _, act1), (w, bias, _), lib, st = layers[0], layers[-1], self.lib, _lib.stream_ptr()

        def middle(n, i, A):
            for li in range(1, len(layers) - 1):
                wl, bl, al = layers[li]
                core.linear_fwd(lib, bufs, A, wl, bl, al, B, wl.shape[0], wl.shape[1], bufs.acts[li], st)
                A = bufs.acts[li]
            return A

        return self._latent_reverse(bufs, ops, T, B, w.shape[1], act1, pre, p, (bufs.acts[0], bufs.lat_h),
                                    middle if len(layers) > 2 else None, e, tabs["c1"], tabs["c2"], w, bias, x_T, **kw)

    def _latent_loop(self, bufs, layers, x_start, csr, steps, T, tabs32, noise0, stop=False, eps=None):
        """The reverse loop in the first hidden layer's space (EngineBase._latent_reverse has the algebra and the loop): here p_T and
        the dense x_T.  x_T is built as in the item-space loop -- same builder, same Philox offsets -- into bufs.xin, and p_T = W1x x_T
        is the first layer on it without time columns and activation (a gather on CSR rows).
        stop: return the engine_core.LatentProduct of the last product without running it; on CSR rows no builder runs then (nothing
        reads a dense x_T) -- the Philox position advances as if it had.  eps (engine_core.EpsTables): the EPSILON target."""
        lib, st, I = self.lib, _lib.stream_ptr(), self.I
        B, dev = x_start.shape[0], x_start.device
        w1 = layers[0][0]
        h1 = w1.shape[0]
        ops, tabs, p, _ = self._latent_begin(bufs, layers, T, B, tabs32)
        t_vec = torch.full((B,), max(steps - 1, 0), dtype=torch.int64, device=dev)
        if csr is not None:
            if stop:
                keep, self.offset = None, self.offset + 1  # (where _prep_csr would have drawn)
            else:
                keep = self._prep_csr(bufs, csr, t_vec, None, None, None, None, False)  # x_T = x_0 (the output product's x_t operand)
            wt = self._transposed(w1)
            core.gather_fwd(lib, None, None, csr, wt, I, None, None, 0, None, 0, B, h1, p, st)
        else:
            ca, cb = (tabs32["sqrt_ab"], tabs32["sqrt_1mab"]) if steps > 0 else (None, None)
            keep = self._prep(bufs, x_start, t_vec, ca, cb, noise0, None, False, xin=bufs.xin)  # x_T
            core.linear_fwd(lib, bufs, (bufs.xin.data_ptr(), bufs.xin.stride(0)), w1, None, 0, B, h1, I, p, st)
        bufs.xin_ones = False
        x0 = self._latent_run(bufs, layers, ops, tabs, T, B, p, p, ops.e, bufs.xin, stop=stop, eps=eps)
        self._saved = None
        del keep
        return x0
