"""One-hot backbone `DNNOneHot` (reference models/DNN.py:360-477) on the HIP path -- first slice of SURVEY 8 f1.

The denoiser has two input branches: [x_t, emb] through `in_layers` and the flattened one-hot rows [x_U (two columns per
item), emb] through `in_layers2`; their hidden activations are concatenated in front of `out_layers`.  It is driven by
`GaussianDiffusionDiscrete(CatOneHot=True)` (gaussian_diffusion.py), whose discrete transition noise on the one-hot rows
is `gdmcf_onehot_noise_f32`.  Everything else is the same C-ABI kernels as the plain DNN: the input builder (once per
branch), the dense layers, the fused loss epilogue, the weight / input gradient GEMMs and the embedding-branch backward
(once per branch, the two `emb_layer` gradients are added).  The concatenation costs nothing: the last layer of each
branch writes straight into its column range of one [B, h1 + h2] buffer, and the gradient of that buffer is read back
by column range.

Training rows may arrive as a `data_utils.CsrBatch` (x0 target, no F.normalize): branch 1 is then fed by
`gdmcf_dnn_prep_input_csr_f32`, branch 2 by `gdmcf_onehot_prep_input_csr_f32` (discrete noise, dropout and embedding columns in
one launch), the loss target is the rows' bitmaps; no dense row and no [B, 2I] image exist, and the Philox positions are
those of the dense route, so the two routes are the same run bit for bit.  `GraphedTrainStep` does not take sparse rows.

The reverse loop takes a `CsrBatch` too where x_T is x_0 (`p_sample` with steps == 0, eval mode, binary rows, no F.normalize,
float32 products; `DNNOneHot` and `DNNOneHotEmbedding`): the one-hot image is then the noiseless one for the whole loop, so the
second branch's first product is `S0 + sum of D[i] over the row's items` plus the step's embedding terms.  That sum is gathered
once per batch (`onehot_rows_sparse` -> `SparseXU`), and per step the layer is one `gdmcf_gather_fwd_f32` launch on it; the
[B, 2I] image and xin2 do not exist, and branch 1's first product at the first step is a gather of the rows' weight rows.

`gemm_dtype="bf16"` rounds the GEMM operands to bf16 on chip (from the f32 tensors: no bf16 shadows here).  Data parallel: the engine hands every gradient to `DataParallelStep`'s sink as soon as its
kernels are enqueued (overlapped all-reduce, or the sharded optimiser with its all-gathers waited for at the end of the
step).  Constructor, parameter names and initialisation draw order are the reference's, so checkpoints interchange.
"""
import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import engine_core as core
from .engine_core import EngineBase, _Bufs, _ceil64, with_precision
from .reverse_route import Carries


class SparseXU:
    """Stands in for the [B, 2I] one-hot image x_U during a reverse loop from CSR rows (OneHotEngine.onehot_rows_sparse): the rows
    (`batch`: data_utils.CsrBatch) and `P2` [B, h], the second branch's first-layer pre-activation without its embedding and bias
    terms -- S0 + sum over the row's items of D[i] -- which is the same at every step of the loop."""

    def __init__(self, batch, P2):
        self.batch, self.P2 = batch, P2
        self.shape, self.device, self.is_cuda = (batch.shape[0], batch.shape[1], 2), batch.device, batch.is_cuda


class _OneHotBufs(_Bufs):
    """xin2 [B, ld2], the second branch's first-layer input, is made on first use: a reverse loop from CSR rows never reads it
    (110 MB at the Yelp shape)."""

    def __getattr__(self, name):  # (only reached while the attribute does not exist yet)
        if name != "xin2":
            raise AttributeError(name)
        self.xin2 = torch.zeros(self.xin1.shape[0], self.ld2, dtype=torch.float32, device=self.xin1.device)
        return self.xin2


class OneHotEngine(EngineBase):
    # -- layers -------------------------------------------------------------------------------------------------------
    def _chains(self):
        m = self.model
        br1 = [(l.weight, l.bias, 1) for l in m.in_layers]
        br2 = [(l.weight, l.bias, 1) for l in m.in_layers2]
        n_out = len(m.out_layers)
        out = [(l.weight, l.bias, 1 if i != n_out - 1 else 0) for i, l in enumerate(m.out_layers)]
        self._check_params(br1 + br2 + out)
        return br1, br2, out

    def buffers(self, B, device):
        key = (B, str(device))
        b = self._bufs.get(key)
        if b is not None:
            return b
        I, E = self.I, self.E
        br1, br2, out = self._chains()
        f32 = dict(dtype=torch.float32, device=device)
        b = _OneHotBufs()
        b.ld1, b.ld2 = _ceil64(I + E), _ceil64(2 * I + E)
        b.xin1 = torch.zeros(B, b.ld1, **f32)
        b.xU = None  # the [B, 2I] one-hot image of the dense route: made on its first step (_xU), never by a run on CSR rows
        b.x0bits = None
        b.h1, b.h2 = br1[-1][0].shape[0], br2[-1][0].shape[0]
        b.hcat = torch.zeros(B, _ceil64(b.h1 + b.h2), **f32)
        b.dhcat = torch.zeros_like(b.hcat)
        mk = lambda chain: [torch.zeros(B, _ceil64(w.shape[0]), **f32) for (w, _, _) in chain[:-1]]
        b.acts1, b.acts2, b.acts_out = mk(br1), mk(br2), mk(out)
        b.dz1, b.dz2, b.dz_out = mk(br1), mk(br2), mk(out)
        b.hs = torch.zeros(B, _ceil64(out[-1][0].shape[1]), **f32)  # row-scaled input of the loss layer (its weight gradient)
        self._shared_buffers(b, B, device, out[-1][0].shape[0], max(br1[0][0].shape[0], br2[0][0].shape[0]),
                             [w for w, _, _ in br1 + br2 + out])
        self._bufs[key] = b
        return b

    # -- input builders ---------------------------------------------------------------------------------------------
    @staticmethod
    def _batch_of(spec):
        """(B, device) of a training step's rows: a dense [B, I] tensor, or a data_utils.CsrBatch under spec["csr"]."""
        x = spec.get("csr")
        x = spec["x_start"] if x is None else x
        return x.shape[0], x.device

    def _xU(self, bufs, B, device):
        if bufs.xU is None:
            bufs.xU = torch.zeros(B, 2 * self.I, dtype=torch.float32, device=device)
        return bufs.xU

    def onehot_rows(self, x0, ts_U, sampled, discrete, out=None):
        """x_tU of the reference (:841-849 / :672-686) as the [B, 2I] float image the second branch reads."""
        B = x0.shape[0]
        x0 = core._f32_rows(x0)
        if out is None:
            out = torch.empty(B, 2 * self.I, dtype=torch.float32, device=x0.device)
        s8 = None
        if sampled is not None:
            s8 = (sampled if sampled.dtype == torch.uint8 else (sampled != 0).to(torch.uint8)).contiguous()
        elif ts_U is not None:
            ts_U = ts_U.to(device=x0.device, dtype=torch.int64).contiguous()
        self.offset += 1
        _lib.check(self.lib.gdmcf_onehot_noise_f32(
            x0.data_ptr(), x0.stride(0), _lib.ptr(ts_U), B, self.I, float(discrete), _lib.ptr(s8),
            s8.stride(0) if s8 is not None else 0, self.seed, self.offset, out.data_ptr(), out.stride(0), None, 0,
            _lib.stream_ptr()))
        return out, (x0, s8, ts_U)

    def _branch2_tables(self, w):
        """(D, S0, tblE) of the second branch's first weight w [N, 2I + E], cached per weight version like _transposed: with
        the noiseless one-hot image of a binary row (column 2i + 1 set for the row's items, column 2i for every other item)
        image @ w^T = S0 + sum over the row's items of D[i], D[i] = w^T[2i + 1] - w^T[2i] ([I, N32], each entry rounded once),
        S0 = sum_i w^T[2i] ([N], summed in float64 and rounded once); tblE [E, N32]: the rows of w^T behind the image."""
        rec = self._wt.get(("br2", id(w)))
        if rec is None or rec[0] is not w or rec[1] != w._version or rec[2][0].device != w.device:
            I, E = self.I, self.E
            n = w.shape[0]
            n32 = (n + 31) // 32 * 32
            wd = w.detach()
            even, odd = wd[:, 0:2 * I:2], wd[:, 1:2 * I:2]
            D = torch.zeros(I, n32, dtype=torch.float32, device=w.device)
            torch.sub(odd.t(), even.t(), out=D[:, :n])
            S0 = even.sum(dim=1, dtype=torch.float64).to(torch.float32).contiguous()
            tblE = torch.zeros(max(E, 1), n32, dtype=torch.float32, device=w.device)
            tblE[:E, :n].copy_(wd[:, 2 * I:2 * I + E].t())
            rec = self._wt[("br2", id(w))] = (w, w._version, (D, S0, tblE))
        return rec[2]

    def onehot_rows_sparse(self, batch):
        """What stands in for onehot_rows(x0, None, x0 != 0, .) -- the noiseless image of a reverse loop with steps == 0 -- when
        the rows are a data_utils.CsrBatch of binary rows: no [B, 2I] image and no xin2; one gather launch
        (gdmcf_gather_fwd_f32, base = S0) leaves the second branch's step-independent pre-activation in the handle."""
        B, dev = batch.shape[0], batch.device
        _, br2, _ = self._chains()
        w = br2[0][0]
        N = w.shape[0]
        D, S0, _ = self._branch2_tables(w)
        P2 = torch.empty(B, _ceil64(N), dtype=torch.float32, device=dev)
        core.gather_fwd(self.lib, None, S0, batch, D, self.I, None, None, 0, None, 0, B, N, P2, _lib.stream_ptr())
        self.sparse_gathers = getattr(self, "sparse_gathers", 0) + 1  # (branch-2 gathers launched: one per loop, not per step)
        return SparseXU(batch, P2)

    def _chain_forward(self, bufs, chain, acts, A, B, last_out):
        """A chain of layers from A: layer li writes acts[li], the one after the last of `acts` writes `last_out`."""
        lib, st = self.lib, _lib.stream_ptr()
        for li, (w, bias, act) in enumerate(chain):
            N, K = w.shape
            out = acts[li] if li < len(acts) else last_out
            core.linear_fwd(lib, bufs, A, w, bias, act, B, N, K, out, st)
            A = out

    def _hidden(self, bufs, br1, br2, out, B, sparse=(None, None)):
        """Both branches into hcat, then all out layers but the last; returns the activation feeding the last layer.
        sparse = (CsrBatch or None, SparseXU or None), reverse loop from CSR rows: with the first, xin1 holds those binary rows
        undropped and branch 1's first layer is a gather of their weight rows; with the second, branch 2's first layer is the
        handle's P2 plus this step's embedding terms and bias (xin2 is not read).  Both through gdmcf_gather_fwd_f32."""
        ld, st = bufs.hcat.stride(0), _lib.stream_ptr()
        x_csr, xU = sparse
        hcat2 = (bufs.hcat.data_ptr() + 4 * bufs.h1, ld)
        if x_csr is not None:
            w, bias, act = br1[0]
            o = bufs.acts1[0] if len(br1) > 1 else bufs.hcat
            self._gather_first_layer(bufs, x_csr, w, bias, act, bufs.xin1, B, o, st)
            self._chain_forward(bufs, br1[1:], bufs.acts1[1:], o, B, bufs.hcat)
        else:
            self._chain_forward(bufs, br1, bufs.acts1, bufs.xin1, B, bufs.hcat)
        if xU is not None:
            w, bias, act = br2[0]
            o = bufs.acts2[0] if len(br2) > 1 else hcat2
            _, _, tblE = self._branch2_tables(w)
            core.gather_fwd(self.lib, xU.P2, None, None, None, self.I, (bufs.xin1.data_ptr() + 4 * self.I, bufs.xin1.stride(0)),
                            tblE, self.E, bias, act, B, w.shape[0], o, st)
            self._chain_forward(bufs, br2[1:], bufs.acts2[1:], o, B, hcat2)
        else:
            self._chain_forward(bufs, br2, bufs.acts2, bufs.xin2, B, hcat2)
        self._chain_forward(bufs, out[:-1], bufs.acts_out, bufs.hcat, B, None)
        return bufs.acts_out[len(out) - 2] if len(out) > 1 else bufs.hcat

    # -- fused training forward / backward ----------------------------------------------------------------------------
    @with_precision
    def train_forward(self, spec):
        return self._train_forward(spec)

    def _train_inputs(self, spec, bufs):
        """Both branch inputs (xin1: noised rows, xin2: one-hot image; dropout, normalize, embedding columns) and the
        loss target.  Returns (x0, target, alpha, rowdiv, keepalive)."""
        if spec.get("csr") is not None:
            return self._train_inputs_csr(spec, bufs)
        x0, ts = spec["x_start"], spec["ts"]
        B, dev = x0.shape[0], x0.device
        x0 = core._f32_rows(x0)
        eps_mode = spec["eps_mode"]
        xt_out = None
        if eps_mode:
            if bufs.xt is None:
                bufs.xt = torch.zeros(B, bufs.ldi, dtype=torch.float32, device=dev)
            xt_out = bufs.xt
        training = self.model.training
        _, s8 = self.onehot_rows(x0, spec["ts_U"], spec["sampled"], spec["discrete"], out=self._xU(bufs, B, dev))
        _, noise, keep1 = self._prep_input(bufs, x0, self.I, bufs.xin1, ts, spec["ca"], spec["cb"], spec["noise"],
                                           spec["drop_mask"], training, xt_out=xt_out)
        _, _, keep2 = self._prep_input(bufs, bufs.xU, 2 * self.I, bufs.xin2, ts, None, None, None, spec["drop_mask_U"], training)
        alpha = None
        if eps_mode:
            target, alpha, rowdiv = self._eps_target(bufs, spec, ts, x0, noise)
        else:
            target, rowdiv = x0, bufs.rowdiv_mse
        return x0, target, alpha, rowdiv, (s8, noise, keep1, keep2)

    def _train_inputs_csr(self, spec, bufs):
        """_train_inputs for rows that stay sparse (spec["csr"]: data_utils.CsrBatch; x0 target, no F.normalize): xin1 and the
        rows' bitmaps (the loss target, bufs.x0bits) from gdmcf_dnn_prep_input_csr_f32, xin2 from
        gdmcf_onehot_prep_input_csr_f32 -- no dense row, no one-hot image.  The Philox position advances as on the dense
        route (class draws, branch 1, branch 2), so both routes draw the same numbers from the same seed."""
        batch, ts, m = spec["csr"], spec["ts"], self.model
        B, I = batch.shape
        dev, st, p, training = batch.device, _lib.stream_ptr(), float(m.drop.p), m.training
        if bufs.x0bits is None:
            bufs.x0bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=dev)
        s8, ts_U, sampled = None, spec["ts_U"], spec["sampled"]
        if sampled is not None:
            s8 = (sampled if sampled.dtype == torch.uint8 else (sampled != 0).to(torch.uint8)).contiguous()
        elif ts_U is not None:
            ts_U = ts_U.to(device=dev, dtype=torch.int64).contiguous()
        self.offset += 3
        off_noise, off1, off2 = self.offset - 2, self.offset - 1, self.offset
        _, noise, keep1 = core.prep_input_csr(self.lib, batch, ts, spec["ca"], spec["cb"], spec["noise"], spec["drop_mask"], p,
                                              training, self.seed, off1, m.emb_layer, self.E, bufs.xin1, bufs.temb, bufs.x0bits, st)
        _, _, keep2 = core.onehot_prep_input_csr(self.lib, batch, ts_U, spec["discrete"], s8, self.seed, off_noise, ts,
                                                 spec["drop_mask_U"], p, training, off2, m.emb_layer, self.E, bufs.xin2,
                                                 bufs.temb, st)
        return None, bufs.x0bits, None, bufs.rowdiv_mse, (batch, s8, ts_U, noise, keep1, keep2)

    def _loss_layer(self, spec, bufs, B, A, W, bias, N, K, target, alpha, rowdiv):
        """Last product fused with the per-row loss, then the float64 loss tail (weights, history FIFO, 1/pt)."""
        lib, st = self.lib, _lib.stream_ptr()
        if spec.get("csr") is not None:  # the target rows are the bitmaps the CSR-fed builder wrote
            core.loss_layer_bits(lib, bufs, A, W, bias, target, alpha, B, N, K, st)
        else:
            core.loss_layer(lib, bufs, A, W, bias, target, alpha, B, N, K, st)
        return core.loss_tail(lib, bufs, spec, B, rowdiv, alpha, st)

    def _train_forward(self, spec):
        B, dev = self._batch_of(spec)
        br1, br2, out = self._chains()
        bufs = self.buffers(B, dev)
        self.version += 1
        x0, target, alpha, rowdiv, keep = self._train_inputs(spec, bufs)
        A = self._hidden(bufs, br1, br2, out, B)
        w, bias, _ = out[-1]
        loss = self._loss_layer(spec, bufs, B, A, w, bias, w.shape[0], w.shape[1], target, alpha, rowdiv)
        self._saved = dict(B=B, bufs=bufs, chains=(br1, br2, out), keepalive=(x0, keep, target, alpha, rowdiv, spec["pt"]))
        return loss

    @with_precision
    def train_backward(self, gloss):
        return self._train_backward(gloss)

    # -- backward building blocks -------------------------------------------------------------------------------------
    def _dense_grads(self, bufs, B, w, bias, dz, rs, A, fs=None):
        """(dW, db) of one layer -- or (None, None) once handed to the data-parallel gradient sink, or (None, db) when
        `fs` (_fused_state(w)) is given: w and its moments are then updated in the product's epilogue."""
        db = torch.empty_like(bias) if bias is not None else None
        dW = torch.empty_like(w) if fs is None else None
        st = _lib.stream_ptr()
        A, scol = self._row_scaled(bufs, B, w.shape[1], A, rs, 0, st)
        self._weight_grad(bufs, B, w, dz, rs, A, scol, dW, db, fs, st)
        if fs is None and self.grad_sink is not None and bias is not None:
            self.grad_sink(w, dW)
            self.grad_sink(bias, db)
            return None, None
        return dW, db

    def _branch_backward(self, bufs, B, chain, acts, dzs, xin, I_cols, dz):
        """One input branch from d(pre-activation of its last layer): hidden layers, then the timestep-embedding columns
        of its first layer.  Returns ([(dW, db)...], dWe, dbe).  A fused weight's product (which overwrites W) runs after
        the kernel that reads W: the input gradient, or the embedding backward's read of the first layer's E columns."""
        m, st = self.model, _lib.stream_ptr()
        grads = [None] * len(chain)
        dWe = dbe = None
        for li in range(len(chain) - 1, -1, -1):
            w, bias, _ = chain[li]
            N, K = w.shape
            fs = self._fused_state(w)
            A_prev = acts[li - 1] if li > 0 else xin
            if fs is None:
                grads[li] = self._dense_grads(bufs, B, w, bias, dz, None, A_prev)
            if li > 0:
                self._input_grad(bufs, B, w, N, K, dz, None, A_prev, chain[li - 1][2], dzs[li - 1], st)
            else:
                dWe, dbe = torch.empty_like(m.emb_layer.weight), torch.empty_like(m.emb_layer.bias)
                core.emb_bwd(self.lib, bufs, dz, w, I_cols, self.E, B, N, dWe, dbe, st)
            if fs is not None:
                grads[li] = self._dense_grads(bufs, B, w, bias, dz, None, A_prev, fs)
            if li > 0:
                dz = dzs[li - 1]
        return grads, dWe, dbe

    def _branches_backward(self, bufs, B, br1, br2):
        """Both branches from bufs.dhcat (gradient of the pre-activations behind hcat[:, :h1+h2]); emb_layer's two
        gradients are added.  Returns the list [dWe, dbe, in_layers..., in_layers2...]."""
        m = self.model
        g1, dWe1, dbe1 = self._branch_backward(bufs, B, br1, bufs.acts1, bufs.dz1, bufs.xin1, self.I, bufs.dhcat)
        g2, dWe2, dbe2 = self._branch_backward(bufs, B, br2, bufs.acts2, bufs.dz2, bufs.xin2, 2 * self.I,
                                               (bufs.dhcat.data_ptr() + 4 * bufs.h1, bufs.dhcat.stride(0)))
        dWe, dbe = dWe1 + dWe2, dbe1 + dbe2
        if self.grad_sink is not None:
            self.grad_sink(m.emb_layer.weight, dWe)
            self.grad_sink(m.emb_layer.bias, dbe)
            dWe = dbe = None
        res = [dWe, dbe]
        for g in g1 + g2:
            res += [g[0], g[1]]
        return res

    def _train_backward(self, gloss):
        """Gradients in model.parameters() order: emb_layer (w, b), in_layers..., in_layers2..., out_layers..."""
        sv = self._saved
        if sv is None:
            raise RuntimeError("gdmcf_amd: train_backward without a preceding training_losses")
        bufs, B = sv["bufs"], sv["B"]
        br1, br2, out = sv["chains"]
        st = _lib.stream_ptr()
        # ---- out layers: from the loss layer down to the concatenated hidden activation
        g_out = [None] * len(out)
        dz, rs = bufs.diff, self._rowscale_of(bufs, gloss)
        for li in range(len(out) - 1, -1, -1):
            w, bias, _ = out[li]
            if li > 0:
                A_prev, act_prev, dprev = bufs.acts_out[li - 1], out[li - 1][2], bufs.dz_out[li - 1]
            else:
                A_prev, act_prev, dprev = bufs.hcat, 1, bufs.dhcat  # both branches end in tanh
            fs = self._fused_state(w)
            if fs is None:
                g_out[li] = self._dense_grads(bufs, B, w, bias, dz, rs, A_prev)
            self._input_grad(bufs, B, w, w.shape[0], w.shape[1], dz, rs, A_prev, act_prev, dprev, st)
            if fs is not None:  # (after the input gradient, which reads w)
                g_out[li] = self._dense_grads(bufs, B, w, bias, dz, rs, A_prev, fs)
            dz, rs = dprev, None
        res = self._branches_backward(bufs, B, br1, br2)
        for g in g_out:
            res += [g[0], g[1]]
        return res

    # -- plain forward (evaluation / reverse loop) ----------------------------------------------------------------------
    def _plain_inputs(self, x, timesteps, x_U, training, drop_mask, drop_mask_U):
        """What every forward_plain starts with: buffers, a new version, both branch inputs built from (x, t) and the
        one-hot image x_U.  Returns (bufs, x, keepalive, sparse).
        Reverse loop from CSR rows (GaussianDiffusionDiscrete.p_sample): x_U is a SparseXU handle -- no xin2 is built, branch 2
        reads the handle -- and at the first step x is the CsrBatch itself: xin1 comes from the CSR-fed builder, and the dense
        x_t the posterior epilogue needs is xin1's first I columns.  `sparse` = (that CsrBatch or None, the handle or None) is
        what _hidden takes."""
        from .data_utils import CsrBatch
        B, dev = x.shape[0], x.device
        bufs = self.buffers(B, dev)
        self.version += 1
        self._saved = None
        ts = timesteps.to(device=dev, dtype=torch.int64).contiguous()
        x_csr = x if isinstance(x, CsrBatch) else None
        xU = x_U if isinstance(x_U, SparseXU) else None
        if (x_csr is not None or xU is not None) and (
                (training and self.model.drop.p > 0) or drop_mask is not None or drop_mask_U is not None or self.model.norm
                or self.gemm_dtype != "f32" or (x_csr is not None and (xU is None or x_csr.csr.values is not None))):
            raise RuntimeError(f"gdmcf_amd.{type(self.model).__name__}: CSR rows enter the plain forward only undropped, binary, "
                               "with norm=False and float32 products (GaussianDiffusionDiscrete.p_sample densifies the rest)")
        if x_csr is not None:
            if bufs.x0bits is None:
                bufs.x0bits = torch.zeros(B, (self.I + 31) // 32, dtype=torch.int32, device=dev)
            self.offset += 1
            m = self.model
            keep1 = core.prep_input_csr(self.lib, x_csr, ts, None, None, None, None, float(m.drop.p), False, self.seed, self.offset,
                                        m.emb_layer, self.E, bufs.xin1, bufs.temb, bufs.x0bits, _lib.stream_ptr())
            x = bufs.xin1[:, : self.I]
        else:
            x = core._f32_rows(x)
            keep1 = self._prep_input(bufs, x, self.I, bufs.xin1, ts, None, None, None, drop_mask, training)
        if xU is not None:
            return bufs, x, (ts, keep1, xU), (x_csr, xU)
        xu = x_U.reshape(B, -1)
        if xu.shape[1] != 2 * self.I:
            raise RuntimeError(f"gdmcf_amd.{type(self.model).__name__}: x_U must hold two columns per item")
        xu = core._f32_rows(xu)
        keep = (keep1, self._prep_input(bufs, xu, 2 * self.I, bufs.xin2, ts, None, None, None, drop_mask_U, training))
        return bufs, x, (ts, keep), (None, None)

    def _last_layer(self, bufs, A, W, bias, act, B, N, K, x_t, posterior):
        """The layer that produces the model output: plain (`out`), or -- reverse loop -- with the posterior mean of
        reference gaussian_diffusion.py:451-471 / :495-498 fused into the GEMM epilogue (`posterior` = dict of per-row
        coefficient vectors c1, c2[, r1, r2][, sigma, z], want_pred): returns (x_{t-1}, pred_xstart or None)."""
        lib, dev, st = self.lib, x_t.device, _lib.stream_ptr()
        if posterior is None:
            res = torch.empty(B, N, dtype=torch.float32, device=dev)
            core.linear_fwd(lib, bufs, A, W, bias, act, B, N, K, res, st)
            return res
        if act != 0:
            raise RuntimeError("fused posterior: the output layer must be linear")
        po = posterior
        xn = torch.empty(B, N, dtype=torch.float32, device=dev)
        pred = torch.empty(B, N, dtype=torch.float32, device=dev) if po.get("want_pred") else None
        core.posterior_fwd(lib, A, W, bias, x_t, po["c1"], po["c2"], po.get("r1"), po.get("r2"), po.get("sigma"), po.get("z"),
                           B, N, K, xn, pred, st)
        return xn, pred

    @with_precision
    def forward_plain(self, x, timesteps, x_U, training, drop_mask=None, drop_mask_U=None, posterior=None):
        br1, br2, out = self._chains()
        bufs, x, keep, sparse = self._plain_inputs(x, timesteps, x_U, training, drop_mask, drop_mask_U)
        B = x.shape[0]
        A = self._hidden(bufs, br1, br2, out, B, sparse)
        w, bias, act = out[-1]
        res = self._last_layer(bufs, A, w, bias, act, B, w.shape[0], w.shape[1], x, posterior)
        del keep
        return res


    # -- reverse loop in the first hidden layer's space (GaussianDiffusionDiscrete.p_sample(latent=True)) ---------------------
    def _latent_second(self, bufs, out):
        """(second [I, K], K, b_out or None, the parameters behind them): the product that turns the last activation into the
        prediction."""
        w, bias, _ = out[-1]
        return w, w.shape[1], bias, (w, bias)

    def _latent_A(self, bufs, out, B, index):
        """The activation that feeds the last product, from bufs.hcat = [h | h_U]."""
        self._chain_forward(bufs, out[:-1], bufs.acts_out, bufs.hcat, B, None)
        return bufs.acts_out[len(out) - 2] if len(out) > 1 else bufs.hcat

    def _set_hcat(self, bufs, t):
        bufs.hcat = t

    @with_precision
    def latent_loop(self, x_T, x_U, T, tabs32, index=None, before_step=None, stop=False, eps=None):
        """The whole reverse loop with x_t carried as p_t = W1x x_t, the first layer of branch 1 without its time columns
        (EngineBase._latent_reverse has the algebra and the loop): per step one step kernel with A = the activation behind
        [h | h_U] that feeds the last product and M = W1x . W_out (an embedding backbone: W1x . V^), plus the small layers.
        Branch 2 sees the same image at every step: its first layer's pre-activation without time columns and bias is taken
        ONCE per call -- from the SparseXU handle, or one product on the dense image -- and re-enters every step through
        gdmcf_gather_fwd_f32 with that step's row of the time table as the bias.  Item-wide work per call: branch 1's first layer
        on x_T (a gather on CSR rows), branch 2's once, and the last product.
        x_T: dense [B, I] rows or a data_utils.CsrBatch of binary rows; x_U: the [B, 2I] image or a SparseXU; tabs32: the
        schedule's float32 tables [T]; before_step(n, i): called ahead of step n (timestep i), e.g. the degree-guided graph update.
        stop (gdmcf_amd.recommend): return the engine_core.LatentProduct of the last product without running it; on CSR rows no
        builder runs then (nothing reads a dense x_T) -- the Philox position advances as if it had.
        eps (engine_core.EpsTables; p_sample(latent="extended")): the EPSILON target."""
        from .data_utils import CsrBatch
        lib, st, I = self.lib, _lib.stream_ptr(), self.I
        B, dev = x_T.shape[0], x_T.device
        br1, br2, out = self._chains()
        bufs = self.buffers(B, dev)
        self.version += 1
        self._saved = None
        if self.model.norm or self.gemm_dtype != "f32":
            raise RuntimeError("gdmcf_amd: the latent reverse loop takes norm=False and float32 products "
                               "(GaussianDiffusion._latent_reverse_ok)")
        if index is not None:
            index = self._index_on(index, dev, B)
        (w1, b1, act1), (w2, b2, act2) = br1[0], br2[0]
        hf1, hf2 = w1.shape[0], w2.shape[0]
        second, K, b_out, behind = self._latent_second(bufs, out)
        m = self.model
        ops = self._latent_operands(w1, b1, second, K, b_out, T, (w1, b1, w2, b2, m.emb_layer.weight, m.emb_layer.bias) + behind,
                                    tables=[(w2, b2, 2 * I)])
        e2 = ops.tabs[0][0]
        tabs = core.step_tables(tabs32, T, B, ("c1", "c2"), bufs.tab_cache)
        if getattr(bufs, "lat_p", None) is None:
            f32 = dict(dtype=torch.float32, device=dev)
            bufs.lat_p = torch.zeros(B, _ceil64(hf1), **f32)
            bufs.lat_hcat = torch.zeros_like(bufs.hcat)
            bufs.lat_P2 = torch.zeros(B, _ceil64(hf2), **f32)
        p = bufs.lat_p
        # p_T and the dense x_T of the last product's epilogue
        if isinstance(x_T, CsrBatch):
            keep = xdense = None
            self.offset += 1  # (the builder's draw, whether it runs or not)
            if not stop:
                if bufs.x0bits is None:
                    bufs.x0bits = torch.zeros(B, (I + 31) // 32, dtype=torch.int32, device=dev)
                ts = torch.full((B,), T - 1, dtype=torch.int64, device=dev)
                keep = core.prep_input_csr(lib, x_T, ts, None, None, None, None, float(m.drop.p), False, self.seed, self.offset,
                                           m.emb_layer, self.E, bufs.xin1, bufs.temb, bufs.x0bits, st)
                xdense = bufs.xin1
            core.gather_fwd(lib, None, None, x_T, self._transposed(w1), I, None, None, 0, None, 0, B, hf1, p, st)
        else:
            keep = xdense = core._f32_rows(x_T)
            core.linear_fwd(lib, bufs, xdense, (w1.data_ptr(), w1.stride(0)), None, 0, B, hf1, I, p, st)
        # branch 2's step-independent pre-activation
        if isinstance(x_U, SparseXU):
            P2 = x_U.P2
        else:
            xu = core._f32_rows(x_U.reshape(B, -1))
            if xu.shape[1] != 2 * I:
                raise RuntimeError(f"gdmcf_amd.{type(m).__name__}: x_U must hold two columns per item")
            P2 = bufs.lat_P2
            core.linear_fwd(lib, bufs, xu, (w2.data_ptr(), w2.stride(0)), None, 0, B, hf2, 2 * I, P2, st)
            keep = (keep, xu)
        # [h | h_U] alternates between two buffers: with one layer in branch 1 and one out layer, the step kernel writes the next
        # step's h into the buffer it is not reading A from
        pair = (bufs.hcat, bufs.lat_hcat)
        ld = bufs.hcat.stride(0)

        def small(n, i, h):
            cur = pair[n % 2]
            self._set_hcat(bufs, cur)
            hcat2 = (cur.data_ptr() + 4 * bufs.h1, ld)
            if len(br1) > 1:
                self._chain_forward(bufs, br1[1:], bufs.acts1[1:], bufs.acts1[0], B, cur)
            o2 = bufs.acts2[0] if len(br2) > 1 else hcat2
            core.gather_fwd(lib, P2, None, None, None, I, None, None, 0, e2[i], act2, B, hf2, o2, st)
            self._chain_forward(bufs, br2[1:], bufs.acts2[1:], o2, B, hcat2)
            return self._latent_A(bufs, out, B, index)

        try:
            return self._latent_reverse(bufs, ops, T, B, K, act1, p, p, pair if len(br1) == 1 else (bufs.acts1[0],) * 2, small, ops.e,
                                        tabs["c1"], tabs["c2"], second, b_out, xdense, stop=stop, eps=eps, before_step=before_step)
        finally:
            self._set_hcat(bufs, pair[0])
            del keep


class DNNOneHot(nn.Module):
    """Drop-in for the reference DNNOneHot (models/DNN.py:360-477).  As there, `out_dims[0]` of the CALLER's list grows
    by the width of the second branch (the reference aliases and mutates it, :384-385)."""
    reverse_carries = Carries("base", True)

    def __init__(self, in_dims, out_dims, emb_size, time_type="cat", norm=False, dropout=0.5, gemm_dtype="f32"):
        super().__init__()
        if gemm_dtype not in ("f32", "bf16", "f32x3"):
            raise ValueError("Unimplemented GEMM input precision %s" % gemm_dtype)
        self.gemm_dtype = gemm_dtype  # "bf16": dense products on the bf16 matrix pipe, f32 accumulate / state (§4.4)
        self.in_dims = in_dims
        self.in_dims2 = list(in_dims)
        self.in_dims2[0] *= 2
        self.out_dims = out_dims
        assert out_dims[0] == in_dims[-1], "In and out dimensions must equal to each other."
        self.time_type = time_type
        self.time_emb_dim = emb_size
        self.norm = norm
        self.emb_layer = nn.Linear(self.time_emb_dim, self.time_emb_dim)
        if self.time_type == "cat":
            in_dims_temp = [self.in_dims[0] + self.time_emb_dim] + list(self.in_dims[1:])
            in_dims_temp2 = [self.in_dims2[0] + self.time_emb_dim] + list(self.in_dims2[1:])
        else:
            raise ValueError("Unimplemented timestep embedding type %s" % self.time_type)
        out_dims_temp = self.out_dims
        out_dims_temp[0] += self.in_dims2[-1]
        self.in_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(in_dims_temp[:-1], in_dims_temp[1:])])
        self.in_layers2 = nn.ModuleList([nn.Linear(a, b) for a, b in zip(in_dims_temp2[:-1], in_dims_temp2[1:])])
        self.out_layers = nn.ModuleList([nn.Linear(a, b) for a, b in zip(out_dims_temp[:-1], out_dims_temp[1:])])
        self.drop = nn.Dropout(dropout)  # holds p; the masks are applied inside the HIP input kernel
        self.init_weights()
        self.lrelu = torch.nn.LeakyReLU(0.1)  # present (and unused) in the reference; kept for pickling parity
        self._engine = None

    def init_weights(self):
        for layer in list(self.in_layers) + list(self.in_layers2) + list(self.out_layers) + [self.emb_layer]:
            fan_out, fan_in = layer.weight.size()
            layer.weight.data.normal_(0.0, np.sqrt(2.0 / (fan_in + fan_out)))
            layer.bias.data.normal_(0.0, 0.001)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = OneHotEngine(self)
        return self._engine

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_engine"] = None
        return state

    def param_list(self):
        return list(self.parameters())

    def fusable_weights(self):
        """The 2-D weights FusedAdamW.fuse_into_backward may update inside the backward pass (DNN: layer_list())."""
        return [l.weight for l in list(self.in_layers) + list(self.in_layers2) + list(self.out_layers)]

    def forward(self, x, timesteps, x_U, drop_mask=None, drop_mask_U=None, posterior=None):
        """model(x_t, t, x_tU) of the reference's evaluation path.  Training goes through
        GaussianDiffusionDiscrete.training_losses (fused forward + loss with its own backward); this plain forward
        carries no autograd graph.  `posterior` (reverse loop, see OneHotEngine._last_layer): return (x_{t-1}, pred_xstart)
        with the posterior mean fused into the output GEMM instead of the raw output."""
        _lib.require_gpu(x, "DNNOneHot input")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()) and self.training:
            raise RuntimeError("gdmcf_amd.DNNOneHot: the plain forward is not differentiable; train through "
                               "GaussianDiffusionDiscrete.training_losses (or call under torch.no_grad())")
        return self.engine.forward_plain(x, timesteps, x_U, self.training, drop_mask, drop_mask_U, posterior=posterior)
