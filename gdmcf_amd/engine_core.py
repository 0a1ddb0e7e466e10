"""What the four denoiser engines share (engine.DenoiserEngine for DNN; onehot.OneHotEngine and its two subclasses):
  * one call helper per C entry point of include/gdmcf_hip.h that more than one engine uses.  A 2-D operand is a tensor, or
    the pair (pointer, leading dimension) where the caller addresses a column range of a buffer; `st` is the stream.
  * `EngineBase`: Philox position, buffer cache, the buffers every backbone has, parameter layout check, the fused
    optimiser's state, the input builder with its Philox step, the weight-gradient step (row scale, product) and the input gradient
    of one layer.
  * the host side of the reverse loop in the first hidden layer's space: `step_tables`, `EpsTables`, `LatentProduct`, and in
    `EngineBase` the cached operands (`_latent_operands`) and the one step loop with its ending (`_latent_reverse`).
  * `TrainLoss`: the autograd function of the fused training loss.
PyTorch is used for device memory and streams only; every arithmetic step is a HIP kernel.
"""
import collections
import ctypes
import functools

import torch

from . import _lib


def _ceil64(n):
    return (int(n) + 63) // 64 * 64


class _Bufs:
    pass


_GEMM_MODES = {k: _lib.CONSTANTS["GDMCF_GEMM_" + k.upper()] for k in ("f32", "bf16", "f32x3")}  # include/gdmcf_hip.h's enum


def with_precision(fn):
    """Runs an engine entry point with the library's per-thread GEMM input precision set to this engine's."""
    @functools.wraps(fn)
    def wrapped(self, *a, **kw):
        prev = self.lib.gdmcf_gemm_precision(_GEMM_MODES[self.gemm_dtype])
        try:
            return fn(self, *a, **kw)
        finally:
            self.lib.gdmcf_gemm_precision(prev)
    return wrapped


def _pl(a):
    """(pointer, leading dimension) of a 2-D operand; (None, 0) for an absent one."""
    if type(a) is tuple:
        return a
    return (None, 0) if a is None else (a.data_ptr(), a.stride(0))


def _f32_rows(t):
    """`t` as float32 with unit column stride (itself when it already is)."""
    return t if t.dtype == torch.float32 and t.stride(-1) == 1 else t.float().contiguous()


# ------------------------------------------------------------------------------------------------------------------
# input builder
# ------------------------------------------------------------------------------------------------------------------
def _prep_modes(B, ca, noise, drop_mask, drop_p, training):
    """(noise_mode, noise, drop_mode, keep): 0 none / 1 given tensor / 2 in-kernel Philox draw, with the given tensors in
    the layout the builders read (float32 noise, uint8 mask)."""
    noise_mode = 0
    if ca is not None:
        noise_mode = 1 if noise is not None else 2
        if noise is not None:
            noise = _f32_rows(noise)
    drop_mode, keep = 0, None
    if drop_mask is not None:
        drop_mode = 1
        keep = drop_mask.reshape(B, -1)
        keep = (keep if keep.dtype == torch.uint8 else (keep != 0).to(torch.uint8)).contiguous()
    elif training and drop_p > 0.0:
        drop_mode = 2
    return noise_mode, noise, drop_mode, keep


def prep_input(lib, x, I, ts, ca, cb, noise, drop_mask, drop_p, training, seed, offset, norm, emb, E, xin, xt_out, temb,
               rownorm, st):
    """gdmcf_dnn_prep_input_f32 on a [B, I] operand: xin = [ drop(normalize(q_sample(x))) | emb(t) | 1 | 0-pad ].  `emb`: the
    timestep-embedding layer (None with E == 0: no embedding columns).  Returns (x, noise, keep) as the kernel reads them:
    the caller keeps them referenced until the stream has consumed them."""
    B = x.shape[0]
    x = _f32_rows(x)
    noise_mode, noise, drop_mode, keep = _prep_modes(B, ca, noise, drop_mask, drop_p, training)
    (nz, ldn), (kp, ldkp), (xi, ldx), (xo, ldxo) = _pl(noise), _pl(keep), _pl(xin), _pl(xt_out)
    _lib.check(lib.gdmcf_dnn_prep_input_f32(
        x.data_ptr(), x.stride(0), _lib.ptr(ts), _lib.ptr(ca), _lib.ptr(cb), noise_mode, nz, ldn, drop_mode, kp, ldkp, drop_p,
        seed, offset, int(bool(norm)), emb.weight.data_ptr() if emb is not None else None,
        emb.bias.data_ptr() if emb is not None else None, E, B, I, xi, ldx, xo, ldxo, _lib.ptr(temb), _lib.ptr(rownorm), st))
    return x, noise, keep


def prep_input_csr(lib, batch, ts, ca, cb, noise, drop_mask, drop_p, training, seed, offset, emb, E, xin, temb, x0bits, st):
    """gdmcf_dnn_prep_input_csr_f32: the same first-layer input straight from the device CSR rows of `batch`
    (data_utils.CsrBatch), whose bitmaps go to `x0bits`.  Returns (batch, noise, keep) to keep referenced."""
    B, I = batch.shape
    noise_mode, noise, drop_mode, keep = _prep_modes(B, ca, noise, drop_mask, drop_p, training)
    (nz, ldn), (kp, ldkp) = _pl(noise), _pl(keep)
    c = batch.csr
    _lib.check(lib.gdmcf_dnn_prep_input_csr_f32(
        c.indptr.data_ptr(), c.indices.data_ptr(), batch.row_ids.data_ptr(), _lib.ptr(ts), _lib.ptr(ca), _lib.ptr(cb),
        noise_mode, nz, ldn, drop_mode, kp, ldkp, drop_p, seed, offset, emb.weight.data_ptr(), emb.bias.data_ptr(), E, B, I,
        xin.data_ptr(), xin.stride(0), temb.data_ptr(), x0bits.data_ptr(), x0bits.stride(0), st))
    return batch, noise, keep


def onehot_prep_input_csr(lib, batch, ts_U, discrete, sampled, seed, offset_noise, ts, drop_mask, drop_p, training,
                          offset_prep, emb, E, xin, temb, st, sampled_out=None, x0bits=None):
    """gdmcf_onehot_prep_input_csr_f32: the second branch's input [ drop(one-hot image under the discrete noise) | emb(t) | 1 |
    0-pad ] straight from the device CSR rows of `batch` -- what gdmcf_onehot_noise_f32 + prep_input on its [B, 2I] image
    leave in `xin`, without that image.  `sampled`: the given classes (uint8 [B, I]) or None (drawn at `offset_noise` from
    ts_U); the dropout draws at `offset_prep`.  Returns (batch, sampled, keep) to keep referenced."""
    B, I = batch.shape
    _, _, drop_mode, keep = _prep_modes(B, None, None, drop_mask, drop_p, training)
    (sp, lds), (kp, ldkp), (so, ldso), (xb, ldb) = _pl(sampled), _pl(keep), _pl(sampled_out), _pl(x0bits)
    c = batch.csr
    _lib.check(lib.gdmcf_onehot_prep_input_csr_f32(
        c.indptr.data_ptr(), c.indices.data_ptr(), batch.row_ids.data_ptr(), _lib.ptr(ts_U), float(discrete), sp, lds, seed,
        offset_noise, so, ldso, _lib.ptr(ts), drop_mode, kp, ldkp, drop_p, offset_prep,
        emb.weight.data_ptr() if emb is not None else None, emb.bias.data_ptr() if emb is not None else None, E, B, I,
        xin.data_ptr(), xin.stride(0), _lib.ptr(temb), xb, ldb, st))
    return batch, sampled, keep


def cat_prep_input_csr(lib, batch, ts_U, discrete, sampled, seed, offset_noise, ts, ca, cb, noise, drop_mask, drop_p, training,
                       offset_prep, cat, emb, E, xin, xt, temb, x0bits, clsbits, st):
    """gdmcf_cat_prep_input_csr_f32: the DNNCat backbone's first-layer input [ drop(cat_layer(x_t, one-hot pair)) | emb(t) | 1 |
    0-pad ] and x_t straight from the device CSR rows of `batch` -- what gdmcf_onehot_noise_f32 (at `offset_noise`) +
    gdmcf_cat_prep_input_f32 (at `offset_prep`) leave on the dense rows, without those rows and without the [B, 2I] image.
    `sampled`: the given classes (uint8 [B, I]) or None (drawn from ts_U); `cat`: the cat layer.  The rows go to `x0bits`, the
    classes to `clsbits` (bitmaps).  Returns (batch, noise, keep, drop_mode): the first three to keep referenced, the last for
    the backward pass, which recomputes a drawn keep-mask."""
    B, I = batch.shape
    noise_mode, noise, drop_mode, keep = _prep_modes(B, ca, noise, drop_mask, drop_p, training)
    (sp, lds), (nz, ldn), (kp, ldkp) = _pl(sampled), _pl(noise), _pl(keep)
    c = batch.csr
    _lib.check(lib.gdmcf_cat_prep_input_csr_f32(
        c.indptr.data_ptr(), c.indices.data_ptr(), batch.row_ids.data_ptr(), _lib.ptr(ts_U), float(discrete), sp, lds,
        offset_noise, ts.data_ptr(), _lib.ptr(ca), _lib.ptr(cb), noise_mode, nz, ldn, drop_mode, kp, ldkp, drop_p, seed,
        offset_prep, cat.weight.data_ptr(), cat.bias.data_ptr(), emb.weight.data_ptr(), emb.bias.data_ptr(), E, B, I,
        xin.data_ptr(), xin.stride(0), xt.data_ptr(), xt.stride(0), temb.data_ptr(), x0bits.data_ptr(), x0bits.stride(0),
        clsbits.data_ptr(), clsbits.stride(0), st))
    return batch, noise, keep, drop_mode


def cat_grad_bits(lib, dxin, xt, x0bits, clsbits, drop_mode, keep, drop_p, seed, offset, B, I, ws, ws_bytes, gw, gb, st):
    """gdmcf_cat_grad_bits_f32: the cat layer's four gradients with the one-hot pair taken from the two bitmaps the CSR-fed
    builder wrote (same arithmetic as gdmcf_cat_grad_f32 on the [B, 2I] image)."""
    (kp, ldkp) = _pl(keep)
    _lib.check(lib.gdmcf_cat_grad_bits_f32(
        dxin.data_ptr(), dxin.stride(0), xt.data_ptr(), xt.stride(0), x0bits.data_ptr(), x0bits.stride(0), clsbits.data_ptr(),
        clsbits.stride(0), drop_mode, kp, ldkp, drop_p, seed, offset, B, I, ws.data_ptr(), ws_bytes, gw.data_ptr(), gb.data_ptr(),
        st))


# ------------------------------------------------------------------------------------------------------------------
# dense layers.  W is [N, K] row-major (rows at least K apart), `bufs` lends the split-K workspace.
# ------------------------------------------------------------------------------------------------------------------
def linear_fwd(lib, bufs, A, W, bias, act, B, N, K, out, st):
    """out = act(A @ W^T + bias)"""
    (a, lda), (w, ldw), (o, ldo) = _pl(A), _pl(W), _pl(out)
    _lib.check(lib.gdmcf_linear_fwd_f32(a, lda, w, ldw, _lib.ptr(bias), act, B, N, K, o, ldo, bufs.ws.data_ptr(),
                                        bufs.ws_bytes, st))


def gather_fwd(lib, pre, base, batch, table, I, a, tblE, E, bias, act, B, N, out, st):
    """gdmcf_gather_fwd_f32: out = act(pre + base + the rows of `table` [I, .] named by the CSR rows of `batch`
    (data_utils.CsrBatch, or None: no gather) + a @ tblE + bias) -- a first layer on a sparse binary input as a sum of rows of the
    transposed weight.  `a` [B, E]: the embedding columns of the builder's xin, read in place; `tblE` [E, .]: their rows of the
    transposed weight.  Every operand but `out` may be None."""
    (p, ldp), (tb, ldt), (ap, lda), (te, ldte), (o, ldo) = _pl(pre), _pl(table), _pl(a), _pl(tblE), _pl(out)
    c = batch.csr if batch is not None else None
    if c is None:
        tb, ldt = None, 0
    if E == 0:
        ap, lda, te, ldte = None, 0, None, 0
    _lib.check(lib.gdmcf_gather_fwd_f32(
        p, ldp, _lib.ptr(base), c.indptr.data_ptr() if c is not None else None, c.indices.data_ptr() if c is not None else None,
        batch.row_ids.data_ptr() if c is not None else None, tb, ldt, I, ap, lda, te, ldte, E, _lib.ptr(bias), act, B, N, o, ldo, st))


def latent_step(lib, A, M, v, p_cur, c1, c2, e, act, B, N, K, p_next, h_next, st):
    """gdmcf_latent_step_f32: p_next = c1 . (A @ M^T + v) + c2 . p_cur, h_next = act(p_next + e) -- one reverse step carried in
    the first hidden layer's space.  M [N, K]; v, e [N] or None; h_next None: not written; p_next may be p_cur."""
    (a, lda), (m, ldm), (pc, ldpc), (pn, ldpn), (h, ldh) = _pl(A), _pl(M), _pl(p_cur), _pl(p_next), _pl(h_next)
    _lib.check(lib.gdmcf_latent_step_f32(a, lda, m, ldm, _lib.ptr(v), pc, ldpc, c1.data_ptr(), c2.data_ptr(), _lib.ptr(e), act,
                                         B, N, K, pn, ldpn, h, ldh, None, 0, st))


def latent_step_ex(lib, A, M, v, p_cur, c1, c2, r, e, act, B, N, K, p_next, h_next, acc, st):
    """gdmcf_latent_step_ex_f32: latent_step with h_next = act((p_next + r) + e) for a row addend r [B, .] (or None) and, with
    acc = (q_cur, qa, qb, q_next), q_next = qa . q_cur + qb . A in the same launch (acc None: no accumulator)."""
    (a, lda), (m, ldm), (pc, ldpc), (pn, ldpn), (h, ldh), (rp, ldr) = _pl(A), _pl(M), _pl(p_cur), _pl(p_next), _pl(h_next), _pl(r)
    (qc, ldqc), (qn, ldqn) = (_pl(acc[0]), _pl(acc[3])) if acc is not None else ((None, 0), (None, 0))
    qa, qb = (acc[1].data_ptr(), acc[2].data_ptr()) if acc is not None else (None, None)
    _lib.check(lib.gdmcf_latent_step_ex_f32(a, lda, m, ldm, _lib.ptr(v), pc, ldpc, c1.data_ptr(), c2.data_ptr(), rp, ldr, _lib.ptr(e),
                                            act, B, N, K, pn, ldpn, h, ldh, qc, ldqc, qa, qb, qn, ldqn, None, 0, st))


def latent_acc(lib, q_cur, qa, A, qb, B, K, q_next, st):
    """gdmcf_latent_acc_f32: q_next = qa . q_cur + qb . A, the accumulator of latent_step_ex as a launch of its own."""
    (qc, ldqc), (a, lda), (qn, ldqn) = _pl(q_cur), _pl(A), _pl(q_next)
    _lib.check(lib.gdmcf_latent_acc_f32(qc, ldqc, qa.data_ptr(), a, lda, qb.data_ptr(), B, K, qn, ldqn, st))


def cand_scores(lib, A, W, I, K, bias, scale, cand, ldcand, B, C, mask_ptrs, rows, out, st):
    """gdmcf_cand_scores_f32: out[b, c] = (A[b, :K] . W[cand[b, c], :K] + bias[cand[b, c]]) * scale[b], -inf for a candidate
    outside [0, I) or in row rows[b] of the mask CSRs.  mask_ptrs: (indptr, indices, indptr2, indices2) device pointers or
    None; cand int64 [B, ldcand] (ldcand 0: one list [C])."""
    (a, lda), (w, ldw), (o, ldo) = _pl(A), _pl(W), _pl(out)
    _lib.check(lib.gdmcf_cand_scores_f32(a, lda, w, ldw, I, K, _lib.ptr(bias), _lib.ptr(scale), cand.data_ptr(), ldcand, B, C,
                                         *mask_ptrs, _lib.ptr(rows), o, ldo, st))


def cand_pick(lib, dense, B, I, scale, cand, ldcand, C, mask_ptrs, rows, out, st):
    """gdmcf_cand_pick_f32: out[b, c] = dense[b, cand[b, c]] * scale[b] under cand_scores' contract."""
    (d, ldd), (o, ldo) = _pl(dense), _pl(out)
    _lib.check(lib.gdmcf_cand_pick_f32(d, ldd, B, I, _lib.ptr(scale), cand.data_ptr(), ldcand, C, *mask_ptrs, _lib.ptr(rows), o,
                                       ldo, st))


def step_tables(tabs32, T, B, names, cache=None):
    """{name: [T, B] float32} of the per-timestep tables `names` of tabs32 (those it holds): row t is the per-row coefficient
    vector of step t as the kernels read it, expanded once instead of per step.  cache: a dict that keeps the last expansion
    per `names`, reused while (tabs32, T, B) stay the same."""
    key = (id(tabs32), int(T), int(B))
    rec = cache.get(names) if cache is not None else None
    if rec is None or rec[0] != key:
        rec = (key, {k: tabs32[k][:T, None].expand(T, B).contiguous() for k in names if k in tabs32})
        if cache is not None:
            cache[names] = rec
    return rec[1]


# A latent reverse loop ended before its last product (stop=True; gdmcf_amd.recommend ranks it): the prediction is
# scale . (A second^T + bias) per row, second [I, K].  x0 target: A = the last activation, bias = b_out, scale = c1[0].
# EPSILON target: A = -Q^, bias = -b_out, scale = D, and the prediction lacks G x_T (EngineBase._latent_reverse).
LatentProduct = collections.namedtuple("LatentProduct", "A second K bias scale")


class EpsTables:
    """Host side of the EPSILON target's latent loop (EngineBase._latent_reverse has the algebra): g_t, d_t, G, D and the
    accumulator's coefficients, formed in float64 from the host's schedule tables and rounded once -- no device read.  g, d: float32
    [T]; qa, qb: float32 [T] (qa[T-1] = 0: Q_T is 0 and is not read; step 0's carry the factor 1 / D); G, D: floats; ok: all
    finite and D > 0."""

    def __init__(self, c1, c2, r1, r2, T):
        import numpy as np
        c1, c2, r1, r2 = (np.asarray(t, dtype=np.float64)[:T] for t in (c1, c2, r1, r2))
        g, d = c1 * r1 + c2, c1 * r2
        G, D = 1.0, 0.0
        with np.errstate(all="ignore"):
            for t in range(T - 1, -1, -1):
                G, D = g[t] * G, g[t] * D + d[t]
            qa, qb = g.copy(), d.copy()
            qa[T - 1] = 0.0
            qa[0], qb[0] = qa[0] / D, qb[0] / D
        self.g, self.d, self.qa, self.qb = (t.astype(np.float32) for t in (g, d, qa, qb))
        self.G, self.D = float(np.float32(G)), float(np.float32(D))
        self.ok = bool(all(np.isfinite(t).all() for t in (self.g, self.d, self.qa, self.qb)) and np.isfinite(self.G)
                       and np.isfinite(self.D) and self.D > 0)
        self._dev = {}  # (device, B) -> the device tables: see on()

    def on(self, device, B):
        """The device tables of one batch size, made once: neg_d, g, qa, qb [T, B]; G, D, qa0_neg, qb0_neg [B]; negative d because
        the step kernel forms c1 (M a + v) + c2 p with c1 := -d, c2 := g."""
        rec, key = self._dev, (str(device), int(B))
        if key not in rec:
            def tab(a):
                return torch.from_numpy(a).to(device)[:, None].expand(len(a), B).contiguous()
            f = dict(dtype=torch.float32, device=device)
            rec[key] = dict(neg_d=tab(-self.d), g=tab(self.g), qa=tab(self.qa), qb=tab(self.qb), G=torch.full((B,), self.G, **f),
                            D=torch.full((B,), self.D, **f), one=torch.ones(B, **f), zero=torch.zeros(B, **f))
            rec[key]["qa0_neg"], rec[key]["qb0_neg"] = -rec[key]["qa"][0], -rec[key]["qb"][0]  # the last step of a stopped loop: -Q^
        return rec[key]


def linear_bwd_input(lib, bufs, dz, W, rs, A_prev, act_prev, B, N, K, d_prev, st):
    """d_prev = ((rs .) dz @ W) * act_prev'(A_prev)"""
    (z, ldz), (w, ldw), (a, lda), (d, ldd) = _pl(dz), _pl(W), _pl(A_prev), _pl(d_prev)
    _lib.check(lib.gdmcf_linear_bwd_input_f32(z, ldz, w, ldw, _lib.ptr(rs), a, lda, act_prev, B, N, K, d, ldd,
                                              bufs.ws.data_ptr(), bufs.ws_bytes, st))


def linear_bwd_weight(lib, dz, A, rs, scol, B, N, K, dW, db, st):
    """dW = dz^T A, db = column sums of dz (out of the product when column K of A holds the row scale: `scol`)"""
    (z, ldz), (a, lda) = _pl(dz), _pl(A)
    _lib.check(lib.gdmcf_linear_bwd_weight_f32(z, ldz, a, lda, _lib.ptr(rs), scol, B, N, K, dW.data_ptr(), dW.stride(0),
                                               _lib.ptr(db), 0, st))


def adamw_args(fs, w):
    """FusedAdamW.fused_state(w) as the argument run (exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step,
    grad_scale) that every kernel with an AdamW epilogue takes."""
    if fs["exp_avg"].stride() != w.stride() or fs["exp_avg_sq"].stride() != w.stride():
        raise RuntimeError("gdmcf_amd: the moments of a fused weight must share its leading dimension")
    return (fs["exp_avg"].data_ptr(), fs["exp_avg_sq"].data_ptr(), fs["lr"], fs["beta1"], fs["beta2"], fs["eps"],
            fs["weight_decay"], fs["step"], fs["grad_scale"])


def dw_adamw_args(dz, A, rs, scol, B, N, K, w, db, fs):
    """Arguments of one fused weight-gradient + AdamW product (w and its moments updated in the epilogue, dW never
    stored): those of gdmcf_linear_bwd_weight_adamw_f32 up to the stream, and the fields of a _lib.GdDwAdamw entry."""
    (z, ldz), (a, lda) = _pl(dz), _pl(A)
    ad = adamw_args(fs, w)
    return (z, ldz, a, lda, _lib.ptr(rs), scol, B, N, K, w.data_ptr(), w.stride(0), ad[0], ad[1], _lib.ptr(db)) + ad[2:]


def linear_bwd_weight_adamw(lib, args, st):
    _lib.check(lib.gdmcf_linear_bwd_weight_adamw_f32(*args, st))


def rowscale(lib, A, rs, B, K, out, st):
    """out[:, :K] = rs . A[:, :K]; a wider `out` also receives rs itself in column K"""
    (a, lda), (o, ldo) = _pl(A), _pl(out)
    _lib.check(lib.gdmcf_rowscale_f32(a, lda, rs.data_ptr(), B, K, o, ldo, st))


def emb_bwd(lib, bufs, dz, W, I_cols, E, B, N, dWe, dbe, st):
    """Gradients of emb_layer from the E timestep-embedding columns (behind column I_cols) of a first layer W [N, .]"""
    (z, ldz), (w, ldw) = _pl(dz), _pl(W)
    _lib.check(lib.gdmcf_emb_bwd_f32(z, ldz, w, ldw, I_cols, E, bufs.temb.data_ptr(), B, N, bufs.demb.data_ptr(),
                                     dWe.data_ptr(), dbe.data_ptr(), st))


# ------------------------------------------------------------------------------------------------------------------
# output layers
# ------------------------------------------------------------------------------------------------------------------
def loss_layer(lib, bufs, A, W, bias, target, alpha, B, N, K, st, reduce=True):
    """Last product fused with the per-row loss: bufs.diff = alpha * (A @ W^T + bias) - target, its row sums of squares in
    bufs.rowsum (the output itself is never stored).  reduce=False: the sums stay partial in bufs.rowpart (loss_tail_job reduces
    them); returns how many there are per row."""
    (a, lda), (w, ldw) = _pl(A), _pl(W)
    _lib.check(lib.gdmcf_linear_loss_fwd_f32(a, lda, w, ldw, _lib.ptr(bias), target.data_ptr(), target.stride(0),
                                             _lib.ptr(alpha), B, N, K, None, 0, bufs.diff.data_ptr(), bufs.ldi,
                                             bufs.rowpart.data_ptr(), bufs.rowsum.data_ptr() if reduce else None, st))
    return int(lib.gdmcf_loss_parts_last())


def loss_layer_bits(lib, bufs, A, W, bias, x0bits, alpha, B, N, K, st, reduce=True):
    """loss_layer with the {0,1} target rows given as bitmaps (the CSR-fed input builders write them): same arithmetic."""
    (a, lda), (w, ldw) = _pl(A), _pl(W)
    _lib.check(lib.gdmcf_linear_loss_fwd_bits_f32(a, lda, w, ldw, _lib.ptr(bias), x0bits.data_ptr(), x0bits.stride(0),
                                                  _lib.ptr(alpha), B, N, K, None, 0, bufs.diff.data_ptr(), bufs.ldi,
                                                  bufs.rowpart.data_ptr(), bufs.rowsum.data_ptr() if reduce else None, st))
    return int(lib.gdmcf_loss_parts_last())


def loss_tail(lib, bufs, spec, B, rowdiv, alpha, st, mean=False):
    """The float64 loss tail (timestep weights, history FIFO, 1/pt) over bufs.rowsum: returns loss [B]; bufs.gradcoef
    receives d(loss_b)/d(rowsum_b).  mean: the tail also emits mean(loss) and, into bufs.rowscale_mean (float32 [B], made on
    first use), gradcoef / B; returns (loss, mean(loss))."""
    ts = spec["ts"]
    loss = torch.empty(B, dtype=torch.float64, device=ts.device)
    args = (bufs.rowsum.data_ptr(), rowdiv.data_ptr(), _lib.ptr(alpha), ts.data_ptr(), spec["weight_t"].data_ptr(),
            spec["pt"].data_ptr(), B, spec["T"], spec["H"], spec["Lt_history"].data_ptr(), spec["Lt_count"].data_ptr(),
            int(spec["update_history"]), bufs.lu.data_ptr(), loss.data_ptr(), bufs.gradcoef.data_ptr())
    if not mean:
        _lib.check(lib.gdmcf_row_loss_finish_f64(*args, st))
        return loss
    loss_mean = torch.empty((), dtype=torch.float64, device=ts.device)
    if getattr(bufs, "rowscale_mean", None) is None:
        bufs.rowscale_mean = torch.zeros(B, dtype=torch.float32, device=ts.device)
    _lib.check(lib.gdmcf_row_loss_finish_mean_f64(*args, loss_mean.data_ptr(), bufs.rowscale_mean.data_ptr(), st))
    return loss, loss_mean


def loss_tail_job(lib, bufs, spec, B, rowdiv, alpha, nt, A, K):
    """What loss_layer(reduce=False) leaves to do, as the tail job of gdmcf_linear_bwd_input_tail_f32: the reduction of the `nt`
    partial sums per row of bufs.rowpart, loss_tail(mean=True), and rowscale(A, bufs.rowscale_mean, B, K, bufs.hs).  Nothing is
    launched here.  Returns (loss, mean(loss), job): the two tensors loss_tail would return -- UNWRITTEN until the job has run
    -- and the _lib.GdKnTail, which keeps `refs` (every tensor it points into) alive."""
    ts = spec["ts"]
    loss = torch.empty(B, dtype=torch.float64, device=ts.device)
    loss_mean = torch.empty((), dtype=torch.float64, device=ts.device)
    if getattr(bufs, "rowscale_mean", None) is None:
        bufs.rowscale_mean = torch.zeros(B, dtype=torch.float32, device=ts.device)
    (a, lda) = _pl(A)
    job = _lib.GdKnTail(bufs.rowpart.data_ptr(), bufs.rowpart.stride(0), nt, bufs.rowsum.data_ptr(), rowdiv.data_ptr(),
                        _lib.ptr(alpha), ts.data_ptr(), spec["weight_t"].data_ptr(), spec["pt"].data_ptr(), spec["T"], spec["H"],
                        spec["Lt_history"].data_ptr(), spec["Lt_count"].data_ptr(), int(spec["update_history"]),
                        bufs.lu.data_ptr(), loss.data_ptr(), bufs.gradcoef.data_ptr(), loss_mean.data_ptr(),
                        bufs.rowscale_mean.data_ptr(), a, lda, bufs.rowscale_mean.data_ptr(), K, bufs.hs.data_ptr(),
                        bufs.hs.stride(0))
    job.refs = (loss, loss_mean, rowdiv, alpha, ts, spec["weight_t"], spec["pt"], spec["Lt_history"], spec["Lt_count"], A)
    return loss, loss_mean, job


def tail_job_run(lib, job, B, st):
    """The three launches of a loss_tail_job on their own (gdmcf_kn_tail_run)."""
    _lib.check(lib.gdmcf_kn_tail_run(ctypes.byref(job), B, st))


def linear_bwd_input_tail(lib, bufs, dz, W, rs, A_prev, act_prev, B, N, K, d_prev, job, st):
    """linear_bwd_input with a loss_tail_job in (or in front of) its launch: gdmcf_linear_bwd_input_tail_f32."""
    (z, ldz), (w, ldw), (a, lda), (d, ldd) = _pl(dz), _pl(W), _pl(A_prev), _pl(d_prev)
    _lib.check(lib.gdmcf_linear_bwd_input_tail_f32(z, ldz, w, ldw, _lib.ptr(rs), a, lda, act_prev, B, N, K, d, ldd,
                                                   bufs.ws.data_ptr(), bufs.ws_bytes, ctypes.byref(job), st))


def posterior_fwd(lib, A, W, bias, x_t, c1, c2, r1, r2, sigma, z, B, N, K, x_next, pred, st):
    """Output layer with the posterior mean of one reverse step (reference gaussian_diffusion.py:451-471 / :495-498) in the
    GEMM epilogue: x_next = c1 * x0_hat + c2 * x_t [+ sigma * z], x0_hat = the output (or r1 * x_t - r2 * output);
    `pred` (optional) receives x0_hat.  The coefficients are per-row vectors [B]."""
    (a, lda), (w, ldw), (zp, ldz), (pp, ldp) = _pl(A), _pl(W), _pl(z), _pl(pred)
    _lib.check(lib.gdmcf_linear_posterior_fwd_f32(
        a, lda, w, ldw, _lib.ptr(bias), x_t.data_ptr(), x_t.stride(0), c1.data_ptr(), c2.data_ptr(), _lib.ptr(r1),
        _lib.ptr(r2), _lib.ptr(sigma), zp, ldz, B, N, K, x_next.data_ptr(), x_next.stride(0), pp, ldp, st))


# ------------------------------------------------------------------------------------------------------------------
class TrainLoss(torch.autograd.Function):
    """loss[B] (float64) of an engine's fused q_sample -> denoiser -> weighted row-MSE path."""

    @staticmethod
    def forward(ctx, eng, spec, *params):
        loss = eng.train_forward(spec)
        ctx.eng, ctx.version = eng, eng.version
        return loss

    @staticmethod
    def backward(ctx, gloss):
        eng = ctx.eng
        if ctx.version != eng.version:
            raise RuntimeError("gdmcf_amd: activations were overwritten by a later forward; "
                               "call backward before the next training_losses/forward")
        return (None, None, *eng.train_backward(gloss))


class EngineBase:
    supports_grad_sink = True  # parallel.DataParallelStep may install `grad_sink` (overlapped gradient exchange)

    def __init__(self, model):
        self.model = model
        self.lib = _lib.load()
        self.E = int(model.time_emb_dim)
        self.I = int(model.in_dims[0])
        self.version = 0
        self.seed = int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        self.offset = 0
        self._bufs = {}
        self._saved = None
        self._wt = {}  # id(weight) -> (weight, version, transposed copy): see _transposed
        self._latent = None  # (key, operands) of the latent reverse loop: see _latent_operands
        # data parallel: called as grad_sink(param, grad) the moment a gradient's kernels are enqueued, so the
        # all-reduce of the big weight gradients overlaps the rest of the backward (gdmcf_amd/parallel.py).
        # When set, the engine assigns .grad itself and hands autograd None for that parameter.
        self.grad_sink = None
        # single-GPU optimiser-in-backward (FusedAdamW.fuse_into_backward): the weights it took over are updated inside the
        # epilogue of the kernel that forms their gradient, which is never materialised (see _fused_state); ignored while a
        # data-parallel grad_sink is installed
        self.fused_opt = None

    @property
    def gemm_dtype(self):
        """"f32": exact-f32 MFMA products (parity path);  "bf16": operands rounded to bf16 on chip, f32 accumulate;
        "f32x3": float32 products from six bf16 MFMAs of three-term operand splits (f32-level error, gemm_split.hip)."""
        return getattr(self.model, "gemm_dtype", "f32")

    def manual_seed(self, seed):
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.offset = 0

    def _check_params(self, layers):
        """`layers`: (weight, bias, activation) of every dense layer, as the kernels read them."""
        what = type(self.model).__name__ + " parameters"
        for w, b, _ in layers:
            _lib.require_gpu(w, what)
            # (rows of a weight may lie further apart than its columns: FusedAdamW.fuse_into_backward seats them on 128-byte lines)
            if not (w.stride(1) == 1 and w.stride(0) >= w.shape[1] and b.is_contiguous() and w.dtype == torch.float32):
                raise RuntimeError(f"gdmcf_amd: {what} must be float32 with unit column stride")

    def _transposed(self, w):
        """W^T of a large weight, [in, out] row-major on 128-byte rows, cached per weight VERSION: the reverse-diffusion loop of an
        evaluation runs many batches over frozen weights, and with the weight in this orientation the hidden layer's product runs
        on the register-streaming kernel (gdmcf_linear_fwd_wt_f32): 0.224 -> 0.205 ms per step at the Yelp shape.  The transpose
        itself (one pass over the weight) is paid once per version.  The same copy is the table of gdmcf_gather_fwd_f32 (the first
        reverse step from CSR rows: its rows are the items', then the E embedding columns')."""
        rec = self._wt.get(id(w))
        if rec is None or rec[0] is not w or rec[1] != w._version or rec[2].device != w.device:
            n, k = w.shape
            buf = torch.zeros(k, (n + 31) // 32 * 32, dtype=torch.float32, device=w.device)
            buf[:, :n].copy_(w.detach().t())
            rec = self._wt[id(w)] = (w, w._version, buf)
        return rec[2]

    def _emb_table(self, w, bias, I_cols, T, st):
        """[T, .] table of a first layer's time columns and bias for every timestep, W_e emb(t) + b with W_e = w[:, I_cols:I_cols + E]:
        gdmcf_dnn_emb_cols_f32 into a scratch input, then gdmcf_gather_fwd_f32 on W_e^T.  Returns (table, scratch to keep)."""
        m, lib, E, h, dev = self.model, self.lib, self.E, w.shape[0], w.device
        f32 = dict(dtype=torch.float32, device=dev)
        e = torch.zeros(T, _ceil64(h), **f32)
        if E == 0:
            e[:, :h].copy_(bias.detach()[None, :].expand(T, h))
            return e, None
        ew, eb = m.emb_layer.weight, m.emb_layer.bias
        # the embedding columns of all T timesteps behind four dummy item columns of a scratch input (16-byte aligned rows)
        xs = torch.zeros(T, _ceil64(4 + E), **f32)
        ts = torch.arange(T, dtype=torch.int64, device=dev)
        temb = torch.zeros(T, E, **f32)
        _lib.check(lib.gdmcf_dnn_emb_cols_f32(ts.data_ptr(), ew.data_ptr(), eb.data_ptr(), E, T, 4, xs.data_ptr(), xs.stride(0),
                                              temb.data_ptr(), st))
        we_t = torch.zeros(E, (h + 3) // 4 * 4, **f32)
        we_t[:, :h].copy_(w.detach()[:, I_cols:I_cols + E].t())
        gather_fwd(lib, None, None, None, None, I_cols, (xs.data_ptr() + 16, xs.stride(0)), we_t, E, bias, 0, T, h, e, st)
        return e, (xs, ts, temb, we_t)

    def _latent_operands(self, w1, bias1, second, K, b_out, T, entering, tables=()):
        """Operands of the reverse loop carried in the first hidden layer's space (gdmcf_latent_step_f32), cached per weight
        VERSION like _transposed -- keyed on (data_ptr, _version, device) of every tensor that enters (`entering`: the
        parameters behind all of the arguments):
          M [h, K] = W1x . second     W1x = w1[:, :I] (read in place, its own leading dimension); second [I, K] = the output layer's
                                      weight (or an embedding backbone's normalised item vectors): gdmcf_linear_bwd_input_f32
          v [h]    = W1x . b_out      (None without b_out): gdmcf_linear_fwd_f32 on the one row b_out
          S [h]    = W1x . 1          the same product on a row of ones (DNNCat from binary CSR rows)
          neg_b [I] = -b_out          (None without b_out) for the eps ranking of gdmcf_amd.recommend
          e [T, h] = W1e emb(t) + b1  the first layer's time columns and bias for every timestep (_emb_table)
          tabs                        the same table for every (weight, bias, item columns) of `tables`
        Returns a _Bufs with M, v, S, neg_b, e, tabs.  One item-wide product per weight version; an evaluation pass pays it once."""
        lib, st = self.lib, _lib.stream_ptr()
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in entering) + (int(T), int(K), b_out is None)
        if self._latent is not None and self._latent[0] == key:
            return self._latent[1]
        h, I, dev = w1.shape[0], self.I, w1.device
        f32 = dict(dtype=torch.float32, device=dev)
        o, ws = _Bufs(), _Bufs()
        ws.ws_bytes = int(max(lib.gdmcf_linear_ws_bytes(h, I, K), lib.gdmcf_linear_ws_bytes(1, h, I)))
        ws.ws = torch.empty(max(ws.ws_bytes, 256), dtype=torch.uint8, device=dev)
        w1x = (w1.data_ptr(), w1.stride(0))
        o.M = torch.zeros(h, _ceil64(K), **f32)
        linear_bwd_input(lib, ws, w1x, second, None, None, 0, h, I, K, o.M, st)
        o.v = o.neg_b = None
        if b_out is not None:
            o.v = torch.zeros(h, **f32)
            linear_fwd(lib, ws, (b_out.data_ptr(), I), w1x, None, 0, 1, h, I, (o.v.data_ptr(), h), st)
            o.neg_b = -b_out.detach()  # the eps ranking of gdmcf_amd.recommend: second (-Q^) + (-b_out), scale D
        # S [h] = W1x . 1 (DNNCat on binary CSR rows: r = (w1 + c) S + (w2 - w1) p_T)
        ones = torch.ones(I, **f32)
        o.S = torch.zeros(h, **f32)
        linear_fwd(lib, ws, (ones.data_ptr(), I), w1x, None, 0, 1, h, I, (o.S.data_ptr(), h), st)
        o.keep_S = ones
        o.e, o.keep = self._emb_table(w1, bias1, I, T, st)
        o.tabs = [self._emb_table(w, b, cols, T, st) for w, b, cols in tables]
        self._latent = (key, o)
        return o

    def _latent_reverse(self, bufs, ops, T, B, K, act, pre, p, hpair, small, e, c1, c2, second, b_out, x_T, stop=False, eps=None,
                        r=None, c1_of=None, before_step=None):
        """The reverse loop carried in the first hidden layer's space, from p_T to x_0: the one step loop and the one
        ending of every backbone's latent loop.
        With the x0 target and no sampling noise the item-space loop is linear in x_t between two hidden activations,
        x_{t-1} = c1[t] (second a_t + b_out) + c2[t] x_t, so p_t = W1x x_t obeys
            p_{t-1} = c1[t] (M a_t + v) + c2[t] p_t,    M = W1x second,  v = W1x b_out,    h_{t-1} = act((p_{t-1} + r) + e_{t-1})
        -- one step kernel per step on the operands of _latent_operands, plus the engine's small layers from h_t to a_t.  Item-wide
        work is left at the two ends, whatever T is: p_T (the engine's, before this call) and the last product,
        x_0 = c1[0] (second a_0 + b_out) -- posterior_mean_coef2[0] is exactly 0.
        eps (EpsTables): the EPSILON target.  The step is x_{t-1} = g_t x_t - d_t (second a_t + b_out) with g_t = c1[t] r1[t] + c2[t],
        d_t = c1[t] r2[t]: the same kernel with c1 := -d, c2 := g.  Unrolled, x_0 = G x_T - D (second Q^ + b_out) with G = prod g_t,
        D <- g_t D + d_t, Q <- g_t Q + d_t a_t and Q^ = Q / D: every step's launch also advances Q (gdmcf_latent_step_ex_f32), step
        0's accumulation is gdmcf_latent_acc_f32 with the factor 1 / D folded in, and x_0 is the posterior epilogue in its eps form
        (r1 = G, r2 = D, c1 = 1, c2 = 0) on the dense x_T.
        The step is gdmcf_latent_step_f32 where there is neither a row addend nor an accumulator, gdmcf_latent_step_ex_f32 otherwise.
          ops            _latent_operands' record (M, v, neg_b);  act: the first layer's activation;  e [T, .]: its time table
          pre, p         [B, .]: the pre-activation of h_{T-1} without e (p_T, plus r where there is one), and the buffer that holds
                         p_T and carries p_t
          hpair          the two buffers the first activation alternates between (one buffer twice where nothing else reads it)
          small(n, i, h) the engine's layers of step n (timestep i) from the first activation h to a_t, the operand of M and second
                         (None: there are none, a_t = h)
          c1, c2         [T, B] posterior_mean_coef1 / 2 (step_tables);  c1_of: maps the step's c1 table (after the eps swap) to the
                         one the kernel reads (DNNCat: times w0)
          r              [B, .] row addend or None;  before_step(n, i): called ahead of step n, e.g. the degree-guided graph update
          x_T            the dense x_T, the x_t operand of the last product's epilogue (x0 target: only finite, c2[0] is 0; eps: it
                         carries G x_T); not read with stop
        Returns x_0 [B, I]; stop: the LatentProduct of the last product instead, which is not run (eps: the sign goes into the last
        accumulation, -Q^ beside the cached -b_out)."""
        lib, st, I, dev, h = self.lib, _lib.stream_ptr(), self.I, p.device, ops.M.shape[0]
        s1, s2, Q = c1, c2, None
        if eps is not None:
            et = eps.on(dev, B)
            s1, s2, qa, qb = et["neg_d"], et["g"], et["qa"], et["qb"]
            if getattr(bufs, "lat_q", None) is None:
                bufs.lat_q = torch.zeros(B, _ceil64(K), dtype=torch.float32, device=dev)
            Q = bufs.lat_q
        if c1_of is not None:
            s1 = c1_of(s1)
        plain = r is None and Q is None
        hcur, hnxt = hpair
        gather_fwd(lib, pre, None, None, None, I, None, None, 0, e[T - 1], act, B, h, hcur, st)  # h_{T-1}
        for n, i in enumerate(range(T - 1, -1, -1)):
            if before_step is not None:
                before_step(n, i)
            A = small(n, i, hcur) if small is not None else hcur
            if i == 0:
                break
            if plain:
                latent_step(lib, A, ops.M, ops.v, p, s1[i], s2[i], e[i - 1], act, B, h, K, p, hnxt, st)
            else:
                latent_step_ex(lib, A, ops.M, ops.v, p, s1[i], s2[i], r, e[i - 1], act, B, h, K, p, hnxt,
                               (Q, qa[i], qb[i], Q) if Q is not None else None, st)
            hcur, hnxt = hnxt, hcur
        if eps is not None:
            qa0, qb0 = (et["qa0_neg"], et["qb0_neg"]) if stop else (qa[0], qb[0])
            latent_acc(lib, Q, qa0, A, qb0, B, K, Q, st)
            if stop:
                return LatentProduct(Q, second, K, ops.neg_b, et["D"])
        elif stop:
            return LatentProduct(A, second, K, b_out, c1[0])
        x0 = torch.empty(B, I, dtype=torch.float32, device=dev)
        if eps is not None:
            posterior_fwd(lib, Q, second, b_out, x_T, et["one"], et["zero"], et["G"], et["D"], None, None, B, I, K, x0, None, st)
        else:
            posterior_fwd(lib, A, second, b_out, x_T, c1[0], c2[0], None, None, None, None, B, I, K, x0, None, st)
        return x0

    @with_precision
    def score_product(self, A, second, K, b_out, B, device):
        """A second^T + b_out into the [B, I] score buffer of this batch size (made on first use, reused by every later call): the
        last product of a latent reverse loop that was ended at its operands (gdmcf_amd.recommend), without the posterior
        epilogue -- c2[0] is 0 and the caller's top-k does not need the factor c1[0]."""
        bufs = self.buffers(B, device)
        if getattr(bufs, "scores", None) is None:
            bufs.scores = torch.empty(B, self.I, dtype=torch.float32, device=device)
        self._grow_workspace(bufs, B, device, [(self.I, K)])
        linear_fwd(self.lib, bufs, A, second, b_out, 0, B, self.I, K, bufs.scores, _lib.stream_ptr())
        return bufs.scores

    def _gather_first_layer(self, bufs, batch, w, bias, act, xin, B, out, st):
        """act([x_0 | emb] @ w^T + bias) for the binary, undropped CSR rows of `batch` as a sum of rows of the cached w^T
        (gdmcf_gather_fwd_f32) instead of the [B, I + E] x [I + E, N] product; `xin` holds this step's embedding columns."""
        N, I, E = w.shape[0], self.I, self.E
        wt = self._transposed(w)
        emb_cols = (xin.data_ptr() + 4 * I, xin.stride(0))
        gather_fwd(self.lib, None, None, batch, wt, I, emb_cols, (wt.data_ptr() + 4 * I * wt.stride(0), wt.stride(0)), E, bias, act,
                   B, N, out, st)

    def _shared_buffers(self, b, B, device, n_loss, n_first, weights):
        """The buffers every backbone has: embedding columns, loss layer, loss tail, embedding backward, GEMM workspace.
        n_loss: columns of the loss layer; n_first: most rows of a first-layer weight; weights: every [N, K] weight that
        goes through the dense layers."""
        lib, I, E = self.lib, self.I, self.E
        f32 = dict(dtype=torch.float32, device=device)
        b.temb = torch.zeros(B, max(E, 1), **f32)
        b.rownorm = torch.zeros(B, **f32)
        b.ldi = _ceil64(I)
        b.diff = torch.zeros(B, b.ldi, **f32)
        b.xt = None
        b.rowpart = torch.zeros(B, lib.gdmcf_loss_tiles(n_loss), **f32)
        b.rowsum = torch.zeros(B, **f32)
        b.gradcoef = torch.zeros(B, **f32)
        b.rowdiv_mse = torch.full((B,), float(I), **f32)
        b.lu = torch.zeros(B, dtype=torch.float64, device=device)
        b.demb = torch.zeros((B + n_first) * max(E, 1), **f32)  # demb [B,E] + gathered W1[:, I:] [n_first,E]
        b.ws_bytes = 0
        b.tab_cache = {}  # step_tables' expansions for this batch size (reverse loops)
        self._grow_workspace(b, B, device, [w.shape for w in weights])

    def _grow_workspace(self, b, B, device, shapes):
        ws = max([b.ws_bytes] + [self.lib.gdmcf_linear_ws_bytes(B, n, k) for n, k in shapes])
        if ws > b.ws_bytes or getattr(b, "ws", None) is None:
            b.ws_bytes = int(ws)
            b.ws = torch.empty(max(ws, 256), dtype=torch.uint8, device=device)

    # -- forward ------------------------------------------------------------------------------------------------------
    def _prep_input(self, bufs, x, I, xin, ts, ca, cb, noise, drop_mask, training, xt_out=None):
        """The input builder on a [B, I] operand at the next Philox position; returns (x, noise, keep) to keep referenced."""
        m = self.model
        self.offset += 1
        return prep_input(self.lib, x, I, ts, ca, cb, noise, drop_mask, float(m.drop.p), training, self.seed, self.offset,
                          m.norm, m.emb_layer, self.E, xin, xt_out, bufs.temb, bufs.rownorm, _lib.stream_ptr())

    def _eps_target(self, bufs, spec, ts, x0, noise):
        """(target, alpha, rowdiv) of the eps parameterisation in one launch (gdmcf_eps_target_f32; reference
        gaussian_diffusion.py:344-348).  A noise tensor this package drew itself (spec["noise_owned"]) IS the target: only its
        t == 0 rows are rewritten; a caller's tensor is left alone."""
        B, dev = ts.shape[0], ts.device
        x0 = _f32_rows(x0)
        target = noise if spec.get("noise_owned", False) else torch.empty(B, self.I, dtype=torch.float32, device=dev)
        alpha = torch.empty(B, dtype=torch.float32, device=dev)
        rowdiv = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.check(self.lib.gdmcf_eps_target_f32(
            noise.data_ptr(), noise.stride(0), bufs.xt.data_ptr(), bufs.xt.stride(0), x0.data_ptr(), x0.stride(0), ts.data_ptr(),
            spec["r1_0"].data_ptr(), spec["r2_0"].data_ptr(), int(bool(spec.get("t0_likelihood", True))), B, self.I,
            target.data_ptr(), target.stride(0), alpha.data_ptr(), rowdiv.data_ptr(), _lib.stream_ptr()))
        return target, alpha, rowdiv

    # -- backward -----------------------------------------------------------------------------------------------------
    def _rowscale_of(self, bufs, gloss):
        """Per-row factor of bufs.diff in the backward: d(total)/d(loss_b) * d(loss_b)/d(rowsum_b)."""
        if isinstance(gloss, float):  # mean reduction: the same upstream gradient 1/B on every row
            return bufs.gradcoef * gloss
        return (gloss.to(torch.float32) * bufs.gradcoef).contiguous()

    def _fused_state(self, w):
        """FusedAdamW.fused_state(w) when the fused optimiser took `w` over (then the caller updates w in the kernel that
        forms its gradient, after every other reader of w in this backward), else None."""
        fused = self.fused_opt if self.grad_sink is None else None
        return fused.fused_state(w) if fused is not None else None

    def _row_scaled(self, bufs, B, K, A, rs, scol, st):
        """First half of a layer's weight-gradient step: (A, scol) as the product reads them.  With a per-row factor `rs`
        on dz, (rs . dZ)^T A == dZ^T (rs . A): the small activation A [B, K] is scaled into bufs.hs instead of the big dZ,
        and the copy's column K (when it has one) holds rs itself, so that db comes out of the product (scol = 1)."""
        if rs is None:
            return A, scol
        rowscale(self.lib, A, rs, B, K, bufs.hs, st)
        return bufs.hs, int(bufs.hs.stride(0) > K)

    def _weight_grad(self, bufs, B, w, dz, rs, A, scol, dW, db, fs, st, queue=None):
        """Second half: the product for w [N, K] from dz = d(loss)/d(pre-activation) up to the per-row factor `rs` (or None)
        and (A, scol) of _row_scaled.  Plain (fs None): dW and db are written.  Fused (fs = _fused_state(w)): w and its
        moments are updated in the product's epilogue, only db is written; with `queue` the product is not launched but
        appended as (GdDwAdamw entry, w) for the caller's gdmcf_linear_bwd_weight_adamw_multi_f32, which then bumps the
        versions."""
        N, K = w.shape
        if fs is None:
            linear_bwd_weight(self.lib, dz, A, rs, scol, B, N, K, dW, db, st)
            return
        args = dw_adamw_args(dz, A, rs, scol, B, N, K, w, db, fs)
        if queue is not None:
            queue.append((_lib.GdDwAdamw(*args), w))
            return
        linear_bwd_weight_adamw(self.lib, args, st)
        # updated through a raw pointer.  bf16 with a registered shadow: the epilogue refreshed the shadow too, and an
        # unchanged version keeps the engine from casting the weight again
        if not (self.gemm_dtype == "bf16" and _lib.shadow_info(w.data_ptr()) is not None):
            torch.autograd.graph.increment_version(w)

    def _input_grad(self, bufs, B, W, N, K, dz, rs, A_prev, act_prev, d_prev, st):
        linear_bwd_input(self.lib, bufs, dz, W, rs, A_prev, act_prev, B, N, K, d_prev, st)
