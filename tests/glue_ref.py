"""Host models of the memory-bound glue kernels (csrc/rows.hip, adamw.hip, loss_tail.hip, dp_exchange.hip, rowscale of
reduce.hip), shared by tests/test_host_glue.py and the GPU modules test_gpu_rows.py, test_gpu_adamw.py, test_gpu_loss_tail.py and
test_gpu_dp_pack.py -- numpy float64 (and exact float32 where a kernel is held to equality), no GPU, no gdmcf_amd import.

  seat / canary_intact     the buffers of every GPU case: NaN where the kernel must write, a canary everywhere else
  densify / csr_case       CSR rows scattered into zeros, and the matrix the densify cases share
  row_loss / kernel_mean   the loss tail in the kernel's own operations and summation order (bit-exact)
  *_bound                  how far a float32 evaluation may be from the float64 reference, each derived in its docstring from
                           the reference's own terms and the summation depth read off the kernel
  adam64 / adam_f32        torch.optim.AdamW's element update in float64, and gd_adam_elem's operations in float32 with a
                           correctly rounded reciprocal and square root (the host check of the bounds)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of float32
CANARY = -77.25  # exact in float32, float64 and (as -77) unlikely in any result
ADAM_C = 1e-6  # see adam_bounds
F32, F64 = np.float32, np.float64


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def seat(rows, width, ld, device, data=None, dtype=torch.float32, offset=0, tail=8):
    """(buf, view): a flat canary-filled buffer and the [rows, width] window of row stride `ld` that starts `offset` elements
    into it; the window holds `data` (a CPU array / tensor), or NaN where a kernel is to write.  `tail` canaries follow the last
    row, so that a store past a row of the last line is seen even with ld == width."""
    assert ld >= width and rows > 0
    fill = CANARY if dtype.is_floating_point else int(CANARY)
    buf = torch.full((offset + rows * ld + tail,), fill, dtype=dtype, device=device)
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :width]
    if data is None:
        view.fill_(float("nan") if dtype.is_floating_point else -(2 ** 62))
    else:
        view.copy_(torch.as_tensor(np.asarray(data)).reshape(rows, width).to(dtype))
    return buf, view


def canary_intact(buf, rows, width, ld, offset=0):
    """True when nothing outside the [rows, width] window of `buf` was written."""
    c = buf.detach().cpu().clone()
    fill = CANARY if c.dtype.is_floating_point else int(CANARY)
    c[offset:offset + rows * ld].view(rows, ld)[:, :width] = fill
    return bool((c == fill).all())


# ---- densify_rows --------------------------------------------------------------------------------------------------------------
def csr_case(I, seed):
    """(indptr int64 [10], indices int32): nine rows over I columns -- unique valid columns per row, and columns -1, I and I + 5 that
    the kernel must skip.  Row 1 is empty, row 2 full, row 4 holds nothing but skipped columns, row 6 is full with skipped ones."""
    rng = np.random.default_rng([seed, I])
    out_of_range = np.array([-1, I, I + 5])
    rows = []
    for r in range(9):
        k = int(rng.integers(1, max(2, min(I, 40))))
        cols = rng.choice(I, size=min(k, I), replace=False)
        if r == 1:
            cols = np.zeros(0, dtype=np.int64)
        if r in (2, 6):
            cols = rng.permutation(I)
        if r == 4:
            cols = out_of_range
        if r in (0, 6, 8):
            cols = np.concatenate([cols[:1], out_of_range[:2], cols[1:], out_of_range[2:]])
        rows.append(cols)
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows).astype(np.int32)


ROW_IDS = (8, 8, 6, 5, 3, 2, 1)  # descending, one repeat; with NULL the rows are 0 .. 6


def densify(indptr, indices, values, row_ids, B, I):
    """float32 [B, I]: row row_ids[b] (b when None) of the CSR matrix scattered into zeros, columns outside [0, I) skipped."""
    out = np.zeros((B, I), dtype=F32)
    for b in range(B):
        u = b if row_ids is None else int(row_ids[b])
        for j in range(int(indptr[u]), int(indptr[u + 1])):
            c = int(indices[j])
            if 0 <= c < I:
                out[b, c] = 1.0 if values is None else values[j]
    return out


# ---- loss tail -----------------------------------------------------------------------------------------------------------------
def row_loss(rowsum, rowdiv, alpha, ts, weight, pt):
    """(loss_unscaled f64, loss f64, gradcoef f32, rowscale_mean f32) of row_loss_finish_kernel, operation by operation.  Every
    step is one IEEE multiplication or division (no addition, so nothing a compiler could contract):
        mse = f32(rowsum) / f32(rowdiv);  lu = weight[ts] * f64(mse);  loss = lu / pt
        gradcoef = f32(((2.0 * alpha) * weight[ts]) / (pt * f64(rowdiv)));  rowscale_mean = gradcoef * (1.0f / f32(B))"""
    rowsum, rowdiv = np.asarray(rowsum, dtype=F32), np.asarray(rowdiv, dtype=F32)
    w = np.asarray(weight, dtype=F64)[np.asarray(ts)]
    pt = np.asarray(pt, dtype=F64)
    mse = rowsum / rowdiv
    assert mse.dtype == F32
    lu = w * mse.astype(F64)
    loss = lu / pt
    a = np.ones(len(rowsum)) if alpha is None else np.asarray(alpha, dtype=F32).astype(F64)
    gc = (((2.0 * a) * w) / (pt * rowdiv.astype(F64))).astype(F32)
    inv_b = F32(1.0) / F32(len(rowsum))
    rsm = gc * inv_b
    assert rsm.dtype == F32
    return lu, loss, gc, rsm


LOSS_B = (1, 63, 64, 65, 255, 256, 257, 400, 1000)
LOSS_TH = ((5, 3), (1000, 10))  # the second needs 88 KB of LDS


def loss_case(B, T, seed, same_ts=False):
    """Inputs of one loss-tail launch: rowsum, rowdiv, alpha (f32 [B]), ts (int64 [B] in [0, T)), weight (f64 [T]), pt (f64 [B])."""
    rng = np.random.default_rng([seed, B, T])
    rowsum = (rng.random(B) * 50 + 0.1).astype(F32)
    rowdiv = np.where(rng.random(B) < 0.5, 1531.0, 3062.0).astype(F32)  # I (mse) or 2 I (likelihood)
    alpha = (rng.random(B) + 0.5).astype(F32)
    ts = rng.integers(0, T, B).astype(np.int64)
    if same_ts:
        ts[:] = ts[0]
    weight = rng.random(T) * 3 + 0.01
    pt = rng.random(B) * 2 + 0.1
    return rowsum, rowdiv, alpha, ts, weight, pt


def kernel_mean(loss, order="kernel"):
    """The float64 mean of row_loss_finish_kernel in its own order: thread t of 256 adds rows t, t + 256, ... onto 0.0; each wave
    of 64 runs the butterfly part += part[lane ^ o] for o = 32 .. 1 (every lane ends with the same sum: a + b == b + a); the four
    wave sums are added as ((s0 + s1) + s2) + s3 and divided by B.  order="pairs" adds them as (s0 + s2) + (s1 + s3) instead --
    the host module uses it to show that the test data tell the two orders apart."""
    loss = np.asarray(loss, dtype=F64)
    B = len(loss)
    padded = np.zeros(-(-B // 256) * 256)  # x + 0.0 == x: rows past B add nothing
    padded[:B] = loss
    part = np.zeros(256)
    for chunk in padded.reshape(-1, 256):
        part = part + chunk
    part = part.reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ o]
    s = part[:, 0]
    total = (s[0] + s[2]) + (s[1] + s[3]) if order == "pairs" else ((s[0] + s[1]) + s[2]) + s[3]
    return total / F64(B)


def kernel_mean_bound(loss):
    """|kernel_mean - exact mean| * B <= B * 2^-53 * sum |loss|: no more than B - 1 + 1 additions and one division lie on any
    path, each with relative error 2^-53 on a partial sum bounded by sum |loss|."""
    loss = np.asarray(loss, dtype=F64)
    return len(loss) * 2.0 ** -53 * float(np.abs(loss).sum())


# ---- derived float32 bounds ------------------------------------------------------------------------------------------------------
def tanh_bwd_ref(dA, A, extra=None, scale=0.0):
    dA, A = np.asarray(dA, dtype=F64), np.asarray(A, dtype=F64)
    g = dA if extra is None else dA + float(scale) * np.asarray(extra, dtype=F64)
    return g * (1.0 - A * A)


def tanh_bwd_bound(dA, extra=None, scale=0.0):
    """out = g f with g = dA + scale * extra and f = 1 - a^2, |g| <= G = |dA| + |scale extra|, f in [0, 1].
      g: the product and the sum round once each (once in all when contracted): |dg| <= 2u G.
      f: a^2 <= 1 rounds with absolute error <= u / 2 (half an ulp below 1), the difference with <= u / 2 more (a single rounding
         of <= u / 2 when contracted to one fma): |df| <= u, well inside the 2u the factor is allowed.
      g f: one rounding, u |g f| <= u G.
    First order: |dg| f + |g| |df| + u G <= (2u + u + u) G = 4u G."""
    mag = np.abs(np.asarray(dA, dtype=F64))
    if extra is not None:
        mag = mag + np.abs(float(scale) * np.asarray(extra, dtype=F64))
    return 4.0 * U * mag


def row_norms_depth(cols):
    """Additions a partial sum of row_norms_kernel passes through: four per 1024-column trip of a thread (three inside the group of
    four squares, one onto the accumulator), then the tail add, block_sum_256's six shuffle adds and three more across the waves --
    the tail add and the last add of the chain are counted in the 9."""
    return 4 * -(-cols // 1024) + 9


def row_norms_rel_bound(cols, inverse=False):
    """All terms are squares, so the sum's relative error is at most (d + 1) u (d additions, one rounding of the square) and the
    square root halves it and adds its own rounding: (d + 1) / 2 + 1 <= d / 2 + 2 units, the half unit to spare covering the
    second-order terms.  1 / norm is one more correctly rounded division."""
    return (row_norms_depth(cols) / 2.0 + 2.0 + (1.0 if inverse else 0.0)) * U


def normalize_bwd_depth(cols):
    """Register branch (cols <= 4096, a multiple of 4): four trips of (three adds inside the group + one onto the accumulator) is
    an upper bound for any term's chain before block_sum_256's nine: 13 counts the accumulator chain (4) and the nine.  Two-pass
    branch: one add per 256-column trip, then the nine."""
    if cols <= 4096 and cols % 4 == 0:
        return 13
    return -(-cols // 256) + 9


def normalize_bwd_ref(dY, Y, rn):
    dY, Y, rn = np.asarray(dY, dtype=F64), np.asarray(Y, dtype=F64), np.asarray(rn, dtype=F64)
    dot = (dY * Y).sum(1, keepdims=True)
    return (dY - Y * dot) * rn[:, None]


def normalize_bwd_bound(dY, Y, rn):
    """dX = (dY - Y dot) rn with dot = sum_i dY_i Y_i.  dot is off by at most (d + 2) u sum_i |dY_i Y_i| (d additions, the
    product's rounding, one to spare), which reaches dX through the factor |Y| rn.  The remaining three roundings (Y dot, the
    difference, the scaling by rn) are each relative to a value bounded by |dY| + |Y dot|: 3u (|dY| + |Y dot|) rn."""
    dY, Y, rn = np.asarray(dY, dtype=F64), np.asarray(Y, dtype=F64), np.asarray(rn, dtype=F64)
    d = normalize_bwd_depth(dY.shape[1])
    dot = (dY * Y).sum(1, keepdims=True)
    mag = np.abs(dY * Y).sum(1, keepdims=True)
    return np.abs(rn)[:, None] * (np.abs(Y) * (d + 2) * U * mag + 3.0 * U * (np.abs(dY) + np.abs(Y * dot)))


def emb_bwd_ref(dZ1, W1, I, E, temb, N):
    """(demb [M, E], dWe [E, E], dbe [E]) in float64."""
    dZ, We, temb = np.asarray(dZ1, dtype=F64)[:, :N], np.asarray(W1, dtype=F64)[:N, I:I + E], np.asarray(temb, dtype=F64)
    demb = dZ @ We
    return demb, demb.T @ temb, demb.sum(0)


def emb_bwd_bounds(dZ1, W1, I, E, temb, N):
    """The same three products with absolute values, times (ceil(N / 64) + ceil(M / 64) + 16) u: a lane of emb_bwd_demb_kernel adds
    ceil(N / 64) products and six shuffle terms, a lane of emb_bwd_w_kernel ceil(M / 64) and six more on top of demb's own error;
    two product roundings and two to spare make 16."""
    M = np.asarray(dZ1).shape[0]
    k = (-(-N // 64) + -(-M // 64) + 16) * U
    dZ, We, temb = np.abs(np.asarray(dZ1, dtype=F64))[:, :N], np.abs(np.asarray(W1, dtype=F64))[:N, I:I + E], np.abs(np.asarray(temb, dtype=F64))
    demb = dZ @ We
    return k * demb, k * (demb.T @ temb), k * demb.sum(0)


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
ADAM_HYPERS = (
    dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=3, grad_scale=0.5),
    dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1, grad_scale=1.0),
    dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, step=100000, grad_scale=0.5),
)
ADAM_NUMELS = (1, 3, 4, 5, 4095, 4096, 4097, 12293)
ADAM_BLOCK = 4096


def adam_state(numel, seed):
    """(p, g, m, v) float32 [numel]: signed weights, gradients and first moments, positive second moments."""
    rng = np.random.default_rng([seed, numel])
    p, g, m = (rng.standard_normal(numel) * 0.05 for _ in range(3))
    v = rng.random(numel) * 1e-3 + 1e-6
    return tuple(x.astype(F32) for x in (p, g, m, v))


def adam64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """torch.optim.AdamW's single-tensor update in float64 from the Python doubles.  Returns (p, m, v, step term, scaled g)."""
    p, g, m, v = (np.asarray(x, dtype=F64) for x in (p, g, m, v))
    g = g * grad_scale
    p = p * (1 - lr * weight_decay)
    m = m * beta1 + (1 - beta1) * g
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    term = lr / bc1 * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p - term, m, v, term, g


def adam_bounds(p, g, m, v, **hyper):
    """(bound_p, bound_m, bound_v) against adam64, g being the scaled gradient:
      m = fma(g - m0, 1 - beta1, m0): the difference, the float32 of 1 - beta1 and the result each round once, the first two
          scaled by 0.1: <= 2u (|m0| + |g|).
      v = fma((1 - beta2) g, g, v0 beta2): two float32 scalars, two products, one result: <= 3u (|v0| + g^2).
      p = fma(neg_step m, rcp(denom), p decay): p decay and the result each round once: 2u |p|; the step term carries the hardware
          reciprocal and square root, documented in csrc/common.h as within ~3e-7 relative of the correctly rounded step, and four
          more float32 roundings (neg_step, its product with m, denom's fma, inv_bc2_sqrt) of 6e-8 each: 5.4e-7, rounded up to
          ADAM_C = 1e-6.  Two terms complete the derivation (without them a correctly rounded float32 evaluation already leaves
          the bound: test_host_glue.py shows it with adam_f32):
            * `decay` is the float32 of the double 1 - lr wd, off by d_decay = |f32(decay) - decay| / decay <= u / 2 (exactly 0
              without weight decay): d_decay |p| more;
            * m's error is bounded in absolute terms (bound_m), not relative to m, which may cancel (0.9 m0 against 0.1 g); it
              reaches p through the step's derivative lr / bc1 / denom: bound_m lr / (bc1 denom) more.
          v's error is relative to v (all its terms are positive), 3u at most, and moves the step by half of that: inside ADAM_C.
    adam_bound_p_as_first_stated returns the parameter bound without the two terms, for the record."""
    p64, m64, v64, term, gs = adam64(p, g, m, v, **hyper)
    bm = 2.0 * U * (np.abs(np.asarray(m, dtype=F64)) + np.abs(gs))
    bv = 3.0 * U * (np.abs(np.asarray(v, dtype=F64)) + gs * gs)
    decay = 1.0 - hyper["lr"] * hyper["weight_decay"]
    d_decay = abs(float(F32(decay)) - decay) / decay
    bc1, bc2 = 1 - hyper["beta1"] ** hyper["step"], 1 - hyper["beta2"] ** hyper["step"]
    denom = np.sqrt(v64) / math.sqrt(bc2) + hyper["eps"]
    bp = (2.0 * U + d_decay) * np.abs(p64) + ADAM_C * np.abs(term) + hyper["lr"] / bc1 / denom * bm
    return bp, bm, bv


def adam_bound_p_as_first_stated(p, g, m, v, **hyper):
    """2u |p| + ADAM_C |step term|: the parameter bound before d_decay and m's propagated error were added (see adam_bounds)."""
    p64, _, _, term, _ = adam64(p, g, m, v, **hyper)
    return 2.0 * U * np.abs(p64) + ADAM_C * np.abs(term)


def _fma32(a, b, c):
    """float32 fma through float64: the product of two float32 is exact in float64; the sum then rounds twice (to 53 bits, to 24),
    which differs from one rounding only on ties of the second -- immaterial for a bound check."""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def adam_f32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """gd_adam_elem's operations in float32 with the scalars of gd_adam_hyper, reciprocal and square root correctly rounded."""
    p, g, m, v = (np.asarray(x, dtype=F32) for x in (p, g, m, v))
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    decay, one_m_b1, one_m_b2 = F32(1.0 - lr * weight_decay), F32(1.0 - beta1), F32(1.0 - beta2)
    inv_bc2_sqrt, neg_step = F32(1.0 / math.sqrt(bc2)), F32(-(lr / bc1))
    g = g * F32(grad_scale)
    p = p * decay
    m = _fma32(g - m, np.full_like(m, one_m_b1), m)
    v = _fma32(one_m_b2 * g, g, v * F32(beta2))
    denom = _fma32(np.sqrt(v), np.full_like(v, inv_bc2_sqrt), np.full_like(v, F32(eps)))
    p = _fma32(neg_step * m, F32(1.0) / denom, p)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def adam_table(numels):
    """(first_block per tensor, total blocks): the prefix sum of ceil(numel / 4096)."""
    first, total = [], 0
    for n in numels:
        first.append(total)
        total += -(-n // ADAM_BLOCK)
    return first, total
