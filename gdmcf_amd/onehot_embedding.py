"""`indexIn` backbone `DNNOneHotEmbedding` (reference models/DNN.py:510-682) on the HIP path -- second slice of SURVEY 8 f1.

Same two input branches as DNNOneHot; instead of `out_layers` (which exist, are initialised and never applied, :582-592
/ :658-662) the concatenation u = [h, h_U, embedding_user(index)] is scored against every row of `embedding_item` by
cosine similarity (:655, :667-682).  With RCloss the NT-Xent term between the two hidden activations (:479-508,
:641-643) is returned too; GaussianDiffusionDiscrete adds 0.1 x it to every row's loss (:952-953).

Device work: the scores are `gdmcf_linear_loss_fwd_f32` (training) / `gdmcf_linear_fwd_f32` (evaluation) on the
row-normalised operands u/|u| and V/|v| (`gdmcf_row_norms_f32` + `gdmcf_rowscale_f32`), their gradients are the usual
input / weight gradient GEMMs followed by the backward of the normalisation (`gdmcf_normalize_rows_bwd_f32`); the user
rows move with `gdmcf_gather_rows_f32` / `gdmcf_scatter_add_rows_f32`; tanh' of the hidden activations takes the NT-Xent
gradient as an addend (`gdmcf_tanh_bwd_f32`).  The NT-Xent term itself is a softmax over a [B, B] matrix of the two
[B, hid] activations -- 0.01 % of the step's arithmetic, but some three dozen eager launches and one stream
synchronisation (`masked_select`) when it is evaluated with the reference's own torch expressions under autograd, which
is what `ntxent="torch"` (the default) does.  `ntxent="fused"` takes the term and its gradient from
`gdmcf_ntxent_fwd_f32` / `gdmcf_ntxent_bwd_f32` (csrc/ntxent.hip; four launches, no synchronisation, no autograd); they
read the two column ranges of `ucat` and write the gradient into the persistent `closs_grad`.  `nt_xent_loss_grad` is the
stand-alone face of the two entries.
"""
import torch
import torch.nn as nn

from . import _lib
from . import engine_core as core
from .engine_core import _ceil64, with_precision
from .onehot import DNNOneHot, OneHotEngine
from .reverse_route import Carries


def nt_xent_loss(z1, z2, temperature=0.1, eps=1e-5):
    """reference models/DNN.py:479-508 (its `loss2`)."""
    n = z1.size(0)
    sim = torch.softmax(torch.mm(z1, z2.t()) / temperature, dim=-1)
    mask = torch.eye(n, device=z1.device).bool()
    negatives = sim.masked_select(~mask).view(n, -1)
    return -torch.log((torch.diag(sim) + eps) / negatives.sum(dim=1)).mean()


NTXENT_MAX_B = 4096  # gdmcf_ntxent_*: 2 <= B <= 4096, 1 <= d <= 4096


@torch.no_grad()
def nt_xent_loss_grad(z1, z2, temperature=0.1, eps=1e-5, scale=None):
    """(loss, dz1, dz2) of `nt_xent_loss(z1, z2, temperature, eps)` without autograd: gdmcf_ntxent_fwd_f32 and
    gdmcf_ntxent_bwd_f32 (four launches, no host synchronisation, same bits in every run).  z1, z2: [B, d] float32 on the
    GPU with unit column stride and any row stride (column ranges of a wider buffer are fine), 2 <= B <= 4096,
    1 <= d <= 4096.  loss: a one-element float32 device tensor; dz1, dz2 [B, d]: scale * d loss / d z, with `scale` a
    one-element float32 device tensor (None: 1)."""
    for t, what in ((z1, "z1"), (z2, "z2")):
        _lib.require_gpu(t, "nt_xent_loss_grad " + what)
        if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1:
            raise ValueError(f"nt_xent_loss_grad: {what} must be a 2-D float32 tensor with unit column stride")
    if z1.shape != z2.shape:
        raise ValueError("nt_xent_loss_grad: z1 and z2 must have the same shape")
    if scale is not None and not (torch.is_tensor(scale) and scale.is_cuda and scale.dtype == torch.float32 and scale.numel() == 1):
        raise ValueError("nt_xent_loss_grad: scale must be a one-element float32 device tensor (or None)")
    lib, st = _lib.load(), _lib.stream_ptr()
    B, d = z1.shape
    f32 = dict(dtype=torch.float32, device=z1.device)
    nbytes = lib.gdmcf_ntxent_ws_bytes(B)
    ws = torch.empty(max(nbytes // 4, 1), **f32)
    loss, dz1, dz2 = torch.empty(1, **f32), torch.empty(B, d, **f32), torch.empty(B, d, **f32)
    _lib.check(lib.gdmcf_ntxent_fwd_f32(z1.data_ptr(), z1.stride(0), z2.data_ptr(), z2.stride(0), B, d, float(temperature),
                                        float(eps), ws.data_ptr(), nbytes, loss.data_ptr(), st))
    _lib.check(lib.gdmcf_ntxent_bwd_f32(z1.data_ptr(), z1.stride(0), z2.data_ptr(), z2.stride(0), B, d, ws.data_ptr(), nbytes,
                                        _lib.ptr(scale), dz1.data_ptr(), dz1.stride(0), dz2.data_ptr(), dz2.stride(0), st))
    return loss, dz1, dz2


class OneHotEmbeddingEngine(OneHotEngine):
    last_ntxent_route = None  # "fused" / "torch": how the last training step evaluated the NT-Xent term

    def buffers(self, B, device):
        b = super().buffers(B, device)
        if hasattr(b, "ucat"):
            return b
        m = self.model
        f32 = dict(dtype=torch.float32, device=device)
        b.h12 = b.h1 + b.h2
        b.eu = m.embedding_user.weight.shape[1]
        b.D = b.h12 + b.eu
        if m.embedding_item.weight.shape != (self.I, b.D):
            raise RuntimeError("gdmcf_amd.DNNOneHotEmbedding: embedding_item must be [n_items, h1 + h2 + user width]")
        ldD = _ceil64(b.D)
        b.ucat = torch.zeros(B, ldD, **f32)   # [h | h_U | user row]; the branches write their column ranges directly
        b.hcat = b.ucat
        b.dhcat = torch.zeros(B, ldD, **f32)  # d(pre-activation) behind ucat[:, :h12]
        b.uhat = torch.zeros(B, ldD, **f32)
        b.du = torch.zeros(B, ldD, **f32)
        b.hs = torch.zeros(B, ldD, **f32)
        b.rn_u = torch.zeros(B, **f32)
        b.rn_v = torch.zeros(self.I, **f32)
        b.Vhat = torch.zeros(self.I, ldD, **f32)
        self._grow_workspace(b, B, device, [(self.I, b.D)])
        return b

    def _ntxent_fused(self, B):
        """B = 1 (the reference's expression then divides by an empty sum) and B > 4096 stay on the torch route."""
        return self.model.ntxent == "fused" and 2 <= B <= NTXENT_MAX_B

    def _ntxent_buffers(self, bufs, B):
        """The fused route's workspace and its persistent gradient buffer, made on the route's first step."""
        if getattr(bufs, "closs_grad", None) is None:
            if bufs.h1 != bufs.h2:
                raise RuntimeError("gdmcf_amd.DNNOneHotEmbedding: the NT-Xent term needs two hidden activations of one width")
            f32 = dict(dtype=torch.float32, device=bufs.ucat.device)
            bufs.ntxent_bytes = self.lib.gdmcf_ntxent_ws_bytes(B)
            bufs.ntxent_ws = torch.empty(bufs.ntxent_bytes // 4, **f32)
            bufs.closs_grad = torch.zeros(B, bufs.ucat.stride(0), **f32)  # [dz1 | dz2] in columns [0, h1), [h1, h12): tanh_bwd's addend
        return bufs.closs_grad

    def _scores_operands(self, bufs, br1, br2, B, index, sparse=(None, None)):
        """ucat = [h, h_U, embedding_user(index)], then the row-normalised operands uhat, Vhat of the cosine scores.
        `sparse`: OneHotEngine._hidden's (reverse loop from CSR rows)."""
        self._hidden(bufs, br1, br2, [None], B, sparse)
        self._user_operand(bufs, B, index)
        self._vhat(bufs)

    def _user_operand(self, bufs, B, index):
        """ucat's user columns = embedding_user(index), then uhat = u / |u| of the scored user vector."""
        lib, st, Wu = self.lib, _lib.stream_ptr(), self.model.embedding_user.weight
        ld = bufs.ucat.stride(0)
        _lib.check(lib.gdmcf_gather_rows_f32(Wu.data_ptr(), Wu.stride(0), index.data_ptr(), B, bufs.eu,
                                             bufs.ucat.data_ptr() + 4 * bufs.h12, ld, st))
        u = self._user_vector(bufs, B)  # what is scored against the items: ucat itself, or a subclass's function of it
        _lib.check(lib.gdmcf_row_norms_f32(u.data_ptr(), u.stride(0), B, bufs.D, None, bufs.rn_u.data_ptr(), st))
        core.rowscale(lib, u, bufs.rn_u, B, bufs.D, bufs.uhat, st)

    def _vhat(self, bufs):
        """V / |v| only changes with the item table (every optimiser step while training; never during evaluation, where
        the reverse loop calls the model T times per batch): rebuilt when the parameter's version counter moved."""
        lib, st, V = self.lib, _lib.stream_ptr(), self.model.embedding_item.weight
        key = (V.data_ptr(), V._version)
        if getattr(bufs, "vhat_key", None) != key:
            _lib.check(lib.gdmcf_row_norms_f32(V.data_ptr(), V.stride(0), self.I, bufs.D, None, bufs.rn_v.data_ptr(), st))
            core.rowscale(lib, V, bufs.rn_v, self.I, bufs.D, bufs.Vhat, st)
            bufs.vhat_key = key

    # -- reverse loop in the first hidden layer's space: pred = uhat . Vhat^T, so M = W1x . Vhat and there is no v --------------
    def _latent_second(self, bufs, out):
        self._vhat(bufs)
        m = self.model
        behind = (m.embedding_item.weight,)  # (what the user vector is made of changes A, not the cached operands)
        return bufs.Vhat, bufs.D, None, behind

    def _latent_A(self, bufs, out, B, index):
        self._user_operand(bufs, B, index)
        return bufs.uhat

    def _set_hcat(self, bufs, t):
        bufs.hcat = bufs.ucat = t

    def _user_vector(self, bufs, B):
        return bufs.ucat

    def _user_vector_backward(self, bufs, B):
        """bufs.du holds the gradient w.r.t. the scored user vector; turn it into the gradient w.r.t. ucat (in place) and
        return {parameter: gradient} of whatever lies between the two."""
        return {}

    @staticmethod
    def _index_on(index, device, B):
        if index is None:
            raise RuntimeError("gdmcf_amd.DNNOneHotEmbedding needs the users' ids (`index`)")
        index = index.to(device=device, dtype=torch.int64).contiguous()
        if index.shape != (B,):
            raise RuntimeError("gdmcf_amd.DNNOneHotEmbedding: `index` must hold one user id per row")
        return index

    def _train_forward(self, spec):
        B, dev = self._batch_of(spec)
        br1, br2, out = self._chains()
        bufs = self.buffers(B, dev)
        self.version += 1
        index = self._index_on(spec["index"], dev, B)
        x0, target, alpha, rowdiv, keep = self._train_inputs(spec, bufs)
        self._scores_operands(bufs, br1, br2, B, index)
        loss = self._loss_layer(spec, bufs, B, bufs.uhat, bufs.Vhat, None, self.I, bufs.D, target, alpha, rowdiv)
        # NT-Xent term between the two hidden activations and its gradient ([B, B] work)
        if self._ntxent_fused(B):
            # csrc/ntxent.hip: reads the two column ranges of ucat, writes closs_grad; no clone, no autograd, no synchronisation
            self.last_ntxent_route = "fused"
            lib, st = self.lib, _lib.stream_ptr()
            ld, cg = bufs.ucat.stride(0), self._ntxent_buffers(bufs, B)
            z1, z2 = bufs.ucat.data_ptr(), bufs.ucat.data_ptr() + 4 * bufs.h1
            closs = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(lib.gdmcf_ntxent_fwd_f32(z1, ld, z2, ld, B, bufs.h1, 0.1, 1e-5, bufs.ntxent_ws.data_ptr(), bufs.ntxent_bytes,
                                                closs.data_ptr(), st))
            _lib.check(lib.gdmcf_ntxent_bwd_f32(z1, ld, z2, ld, B, bufs.h1, bufs.ntxent_ws.data_ptr(), bufs.ntxent_bytes, None,
                                                cg.data_ptr(), cg.stride(0), cg.data_ptr() + 4 * bufs.h1, cg.stride(0), st))
            self.last_closs = closs
        else:
            # the reference's torch expressions under autograd (masked_select synchronises the stream)
            self.last_ntxent_route = "torch"
            with torch.enable_grad():
                h = bufs.ucat[:, : bufs.h1].detach().clone().requires_grad_(True)
                hU = bufs.ucat[:, bufs.h1: bufs.h12].detach().clone().requires_grad_(True)
                closs = nt_xent_loss(h, hU)
                dh, dhU = torch.autograd.grad(closs, (h, hU))
            self.last_closs = closs.detach()
            cg = torch.cat([dh, dhU], dim=1).contiguous()
        self._saved = dict(B=B, bufs=bufs, chains=(br1, br2, out), index=index, closs_grad=cg,
                           keepalive=(x0, keep, target, alpha, rowdiv, spec["pt"]))
        return loss + self.last_closs * 0.1  # reference :952-953 (after the history update and the division by pt)

    def _train_backward(self, gloss):
        """Gradients in model.parameters() order: emb_layer, in_layers, in_layers2, out_layers (None: never applied),
        embedding_item, embedding_user."""
        sv = self._saved
        if sv is None:
            raise RuntimeError("gdmcf_amd: train_backward without a preceding training_losses")
        lib, st, m = self.lib, _lib.stream_ptr(), self.model
        bufs, B, index = sv["bufs"], sv["B"], sv["index"]
        br1, br2, out = sv["chains"]
        rs = self._rowscale_of(bufs, gloss)
        # every row's loss carries + 0.1 * closs: d(total)/d(closs) = 0.1 * sum of the upstream row gradients
        if isinstance(gloss, float):
            gc = torch.full((1,), 0.1 * gloss * B, dtype=torch.float32, device=bufs.ucat.device)
        else:
            gc = (0.1 * gloss.sum()).to(torch.float32).reshape(1)
        V, Wu = m.embedding_item.weight, m.embedding_user.weight
        # fused optimiser: neither table is read again in this backward (the products below read Vhat), so each is updated
        # by the pass that forms its gradient
        fsV, fsU = self._fused_state(V), self._fused_state(Wu)
        # scores = uhat @ Vhat^T: gradient w.r.t. Vhat, then through V / |v|
        dV, _ = self._dense_grads(bufs, B, V, None, bufs.diff, rs, bufs.uhat)
        if fsV is None:
            _lib.check(lib.gdmcf_normalize_rows_bwd_f32(dV.data_ptr(), dV.stride(0), bufs.Vhat.data_ptr(), bufs.Vhat.stride(0),
                                                        bufs.rn_v.data_ptr(), self.I, bufs.D, dV.data_ptr(), dV.stride(0), st))
        else:
            _lib.check(lib.gdmcf_normalize_rows_bwd_adamw_f32(
                dV.data_ptr(), dV.stride(0), bufs.Vhat.data_ptr(), bufs.Vhat.stride(0), bufs.rn_v.data_ptr(), self.I, bufs.D,
                V.data_ptr(), V.stride(0), *core.adamw_args(fsV, V), st))
            torch.autograd.graph.increment_version(V)  # (also what rebuilds the cached V / |v| at the next forward)
            dV = None
        # ... w.r.t. uhat, then through u / |u|
        self._input_grad(bufs, B, bufs.Vhat, self.I, bufs.D, bufs.diff, rs, bufs.ucat, 0, bufs.du, st)
        _lib.check(lib.gdmcf_normalize_rows_bwd_f32(bufs.du.data_ptr(), bufs.du.stride(0), bufs.uhat.data_ptr(),
                                                    bufs.uhat.stride(0), bufs.rn_u.data_ptr(), B, bufs.D, bufs.du.data_ptr(),
                                                    bufs.du.stride(0), st))
        self._extra_grads = self._user_vector_backward(bufs, B)
        # user rows: scatter into the dense table gradient (torch.optim.AdamW on nn.Embedding sees a dense gradient too) --
        # or, fused, one AdamW pass over the whole table that takes the batch rows' gradient straight from du
        if fsU is None:
            dWu = torch.zeros_like(Wu)
            _lib.check(lib.gdmcf_scatter_add_rows_f32(bufs.du.data_ptr() + 4 * bufs.h12, bufs.du.stride(0), index.data_ptr(), B,
                                                      bufs.eu, dWu.data_ptr(), dWu.stride(0), st))
        else:
            _lib.check(lib.gdmcf_scatter_rows_adamw_f32(
                bufs.du.data_ptr() + 4 * bufs.h12, bufs.du.stride(0), index.data_ptr(), B, Wu.shape[0], bufs.eu, Wu.data_ptr(),
                Wu.stride(0), *core.adamw_args(fsU, Wu), st))
            torch.autograd.graph.increment_version(Wu)
            dWu = None
        # hidden activations: + NT-Xent gradient, times tanh'
        cg = sv["closs_grad"]
        _lib.check(lib.gdmcf_tanh_bwd_f32(bufs.du.data_ptr(), bufs.du.stride(0), bufs.ucat.data_ptr(), bufs.ucat.stride(0),
                                          cg.data_ptr(), cg.stride(0), gc.data_ptr(), B, bufs.h12, bufs.dhcat.data_ptr(),
                                          bufs.dhcat.stride(0), st))
        res = self._branches_backward(bufs, B, br1, br2)
        res += [None, None] * len(out)
        if self.grad_sink is not None:
            self.grad_sink(V, dV)
            self.grad_sink(Wu, dWu)
            dV = dWu = None
        sv["keepalive"] = (sv["keepalive"], gc)
        return res + [dV, dWu]

    @with_precision
    def forward_plain(self, x, timesteps, x_U, training, drop_mask=None, drop_mask_U=None, index=None, posterior=None):
        br1, br2, _ = self._chains()
        B = x.shape[0]
        index = self._index_on(index, x.device, B)
        bufs, x, keep, sparse = self._plain_inputs(x, timesteps, x_U, training, drop_mask, drop_mask_U)
        self._scores_operands(bufs, br1, br2, B, index, sparse)
        res = self._last_layer(bufs, bufs.uhat, bufs.Vhat, None, 0, B, self.I, bufs.D, x, posterior)
        del keep
        return res


class DNNOneHotEmbedding(DNNOneHot):
    """Drop-in for the reference DNNOneHotEmbedding (models/DNN.py:510-682); main.py:239-242 builds it with
    `item_num=n_item, user_num=n_user` and sets `diffusion.indexIn = True`."""
    reverse_carries = Carries("base", True)

    def __init__(self, in_dims, out_dims, emb_size, time_type="cat", norm=False, dropout=0.5, item_num=2810, user_num=5949,
                 gemm_dtype="f32", ntxent="torch"):
        if ntxent not in ("torch", "fused"):
            raise ValueError("ntxent must be 'torch' (the reference's expressions under autograd) or 'fused' (csrc/ntxent.hip), "
                             "not %r" % (ntxent,))
        self._defer_init = True
        super().__init__(in_dims, out_dims, emb_size, time_type=time_type, norm=norm, dropout=dropout, gemm_dtype=gemm_dtype)
        self.ntxent = ntxent  # how a training step evaluates the NT-Xent term and its gradient
        eu = self.in_layers[-1].out_features
        self.embedding_item = nn.Embedding(item_num, eu + eu + self.in_layers2[-1].out_features)
        self.embedding_user = nn.Embedding(user_num, eu)
        self.all_indices_item = torch.arange(item_num)
        self.all_indices_user = torch.arange(user_num)
        self._defer_init = False
        self.init_weights()
        self.lrelu = torch.nn.LeakyReLU(0.1)

    def init_weights(self):
        if getattr(self, "_defer_init", False):  # the reference draws once, after the embedding tables exist (:556)
            return
        super().init_weights()
        nn.init.xavier_uniform_(self.embedding_item.weight)
        nn.init.xavier_uniform_(self.embedding_user.weight)

    @property
    def engine(self):
        if self._engine is None:
            self._engine = OneHotEmbeddingEngine(self)
        return self._engine

    def fusable_weights(self):
        """As DNNOneHot's, without `out_layers` (never applied, no gradient), with the two embedding tables."""
        return ([l.weight for l in list(self.in_layers) + list(self.in_layers2)]
                + [self.embedding_item.weight, self.embedding_user.weight])

    @torch.no_grad()
    def load_lightgcn_embeddings(self, lightgcn, users=True, items=True):
        """Hand-off of the LightGCN propagation into the denoiser (the reference's script only saves
        final_user_Embed / final_item_Embed, lightGCN.py:305-323, and nothing reads them).  The propagated tables
        mean_l(A~^l E0) (HIP SpMM, gdmcf_amd.LightGCN.propagate_through_layers) initialise the tables this backbone
        conditions on (reference models/DNN.py:1148-1149, read at :1263-1265 / :1274):
          embedding_user.weight          <- final_user                       (the user row appended to [h, h_U], :1274)
          embedding_item.weight[:, -w:]  <- final_item, w = user width       (the columns that meet the user row in the
                                                                              cosine score, :1288-1289)
        so that score(u, i) contains <e_u, e_i> of the graph model from the first step on.  Needs latent_dim == the user
        embedding width (in_dims[-1] by construction, :1144).  Returns (final_user, final_item)."""
        fu, fi, _, _ = lightgcn.propagate_through_layers()
        wu = self.embedding_user.weight
        if users:
            if fu.shape != wu.shape:
                raise ValueError(f"LightGCN user table {tuple(fu.shape)} does not fit embedding_user {tuple(wu.shape)}")
            wu.copy_(fu)
        if items:
            wi = self.embedding_item.weight
            if fi.shape != (wi.shape[0], wu.shape[1]):
                raise ValueError(f"LightGCN item table {tuple(fi.shape)} does not fit the last {wu.shape[1]} columns of "
                                 f"embedding_item {tuple(wi.shape)}")
            wi[:, wi.shape[1] - wu.shape[1]:].copy_(fi)
        for p_ in (self.embedding_user.weight, self.embedding_item.weight):
            torch.autograd.graph.increment_version(p_)  # cached V/|v| and shadows are keyed on the version counter
        return fu, fi

    def forward(self, x, timesteps, x_U, index=None, graph=None, RCloss=False, drop_mask=None, drop_mask_U=None, posterior=None):
        """model(x_t, t, x_tU, index=..., graph=...) of the reference's evaluation path (`graph` is accepted and, as in the
        reference, unused).  Training goes through GaussianDiffusionDiscrete.training_losses.  `posterior`: see
        DNNOneHot.forward (the reverse loop's posterior mean fused into the score GEMM)."""
        _lib.require_gpu(x, "DNNOneHotEmbedding input")
        if RCloss or (torch.is_grad_enabled() and self.training and any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("gdmcf_amd.DNNOneHotEmbedding: the plain forward is not differentiable and carries no "
                               "NT-Xent term; train through GaussianDiffusionDiscrete.training_losses")
        return self.engine.forward_plain(x, timesteps, x_U, self.training, drop_mask, drop_mask_U, index=index, posterior=posterior)
