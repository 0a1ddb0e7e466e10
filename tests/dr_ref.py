"""Host models of the register-streaming weight-gradient kernels (csrc/gemm_dr_tn.hip: dr_tn_kernel, dr_tn_adamw_kernel) and of
the split-K input gradient (csrc/gemm_dr_kn.hip: dr_kn_kernel), shared by tests/test_host_dr_ref.py and tests/test_gpu_dr_edges.py
-- numpy, no GPU, no gdmcf_amd import.

  dr_tn_plan / CASES     what dr_tn_prepare derives from the batch row count B, and the twelve batches the GPU module sweeps
  dw_operands            the operands of a case (float32, seeded by the shape)
  product_ref / _bound   the float64 product and the element-wise bound a float32 evaluation in ANY order must meet
  chained_f32            the product in float32 in the kernels' k order (the host check that the reference alone passes)
  kn_plan                splits and chunks per split of dr_kn_kernel, and the slabs it writes
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
F32, F64 = np.float32, np.float64


def cdiv(a, b):
    return -(-a // b)


# ---- dr_tn_prepare ---------------------------------------------------------------------------------------------------------------
def dr_tn_plan(B):
    """(D, ksp, waste, rounds, stream) for a reduction over B batch rows: a k-step is 4 rows, a tile runs a multiple of the ring
    size R = D + 1 steps, the depth among 9, 8, 7 that pads the fewest steps wins and ties go to the deeper ring.  `waste` steps read
    past the operands; `stream`: a fused product's AdamW update runs inside the next tile's k loop (>= 9 ring rounds, two of the
    sixteen row groups issued in each of rounds 0..7, the last consumed in round 8), else at the end of its own tile."""
    ks = cdiv(B, 4)
    D, waste = 9, 1 << 30
    for d in (9, 8, 7):
        w = cdiv(ks, d + 1) * (d + 1) - ks
        if w < waste:
            D, waste = d, w
    ksp = ks + waste
    rounds = ksp // (D + 1)
    return D, ksp, waste, rounds, rounds >= 9


# B: (D, ksp, waste, rounds, B % 4) -- written out by hand from the predicate, pinned against dr_tn_plan and the library
CASES = {
    128: (7, 32, 0, 4, 0),
    130: (8, 36, 3, 4, 2),
    145: (9, 40, 3, 4, 1),
    288: (8, 72, 0, 8, 0),
    300: (9, 80, 5, 8, 0),
    320: (9, 80, 0, 8, 0),
    321: (8, 81, 0, 9, 1),
    325: (7, 88, 6, 11, 1),
    357: (9, 90, 0, 9, 1),
    390: (8, 99, 1, 11, 2),
    400: (9, 100, 0, 10, 0),
    512: (7, 128, 0, 16, 0),
}
STREAM_ROUNDS = 9


# ---- operands, reference, bound --------------------------------------------------------------------------------------------------
def dw_operands(B, N, K, seed=0):
    """(dZ [B, N], A [B, K], rs [B]) float32 of dW[N, K] = dZ^T A, db[N] = sum_m rs[m] dZ[m, n]: signed, no zeros, magnitudes as
    in training (dZ ~ 0.1, A ~ 1)."""
    rng = np.random.default_rng([seed, B, N, K])
    dZ = (rng.standard_normal((B, N)) * 0.1).astype(F32)
    A = rng.standard_normal((B, K)).astype(F32)
    rs = (rng.random(B) + 0.5).astype(F32)
    return dZ, A, rs


def product_ref(P, Q):
    """(P^T Q, |P|^T |Q|) in float64 for P [B, n], Q [B, k]."""
    P, Q = np.asarray(P, dtype=F64), np.asarray(Q, dtype=F64)
    return P.T @ Q, np.abs(P).T @ np.abs(Q)


def product_bound(depth, absprod):
    """|float32 sum of `depth` products, in any order, fused or not - exact| <= (depth + 8) u sum |terms|.

    A term passes through its own product rounding (none when fused) and through at most depth - 1 additions before the result,
    whatever the order -- chained, in groups of four, as a tree or over split-K partial sums, which only shorten the chains --:
    each rounding is relative to a partial sum bounded by sum |terms|, so to first order the error is at most depth u sum |terms|
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5 with gamma_n ~ n u).  The eight units on top cover the second-
    order terms (depth^2 u^2 / 2 < u for depth < 5792) and the rounding of the float32 the result is stored as."""
    return (depth + 8) * U * np.asarray(absprod, dtype=F64)


def chained_f32(P, Q):
    """P^T Q in float32 in the kernels' k order: one accumulator per element, the k-steps of four rows in ascending order, the four
    products of a step added onto the accumulator one after the other, each as one fused multiply-add (a float32 product is exact
    in float64; the sum then rounds to 53 and to 24 bits, which differs from a single rounding only on ties of the second)."""
    P, Q = np.asarray(P, dtype=F32), np.asarray(Q, dtype=F32)
    acc = np.zeros((P.shape[1], Q.shape[1]), dtype=F32)
    for k in range(P.shape[0]):
        acc = (acc.astype(F64) + np.outer(P[k].astype(F64), Q[k].astype(F64))).astype(F32)
    return acc


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; inf when anything is not finite"""
    got = np.asarray(got, dtype=F64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / bound).max())


# ---- AdamW gates -----------------------------------------------------------------------------------------------------------------
def adam64(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """torch.optim.AdamW's single-tensor update in float64, written as tests/test_gpu_fullsize.py writes it."""
    p, g, m, v = (np.asarray(x, dtype=F64) for x in (p, g, m, v))
    g = g * grad_scale
    p = p * (1 - lr * weight_decay)
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** step)) * m / (np.sqrt(v) / (1 - beta2 ** step) ** 0.5 + eps)
    return p, m, v


def adam_state(N, K, seed=0):
    """(W, exp_avg, exp_avg_sq) float32 [N, K]: signed weights and first moments, second moments in [1e-6, 1e-3] as
    glue_ref.adam_state's.  The floor keeps the update well conditioned: the step is lr' m / (sqrt(v) / sqrt(bc2) + eps), and where
    v0 and the gradient are both next to zero its derivative by the gradient, lr' (1 - beta1) grad_scale / denom, exceeds 0.1 --
    the float32 rounding of the gradient itself (~1e-5 absolute here) then moves W by more than any tolerance stated relative to
    max |W|, in a correct kernel and in gdmcf_adamw_f32 alike.  (Seen with a floor of 0 at B = 320: v0 = 2.8e-9 beside a gradient of
    2.8e-3 put W 1.7e-6 from float64 against a tolerance of 1.0e-6 -- in the fused kernel and in gdmcf_adamw_f32 on the plain
    entry's dW, which agreed bit for bit.)  With v >= 1e-6 the derivative stays below 0.02."""
    rng = np.random.default_rng([seed, N, K, 7])
    W0 = (rng.standard_normal((N, K)) * 0.05).astype(F32)
    m0 = (rng.standard_normal((N, K)) * 0.01).astype(F32)
    v0 = (rng.random((N, K)) * 1e-3 + 1e-6).astype(F32)
    return W0, m0, v0


# ---- dr_kn_kernel ----------------------------------------------------------------------------------------------------------------
def kn_plan(M, N, K, n_cu):
    """(splits, cps, asked) of dA[M, K] = dZ[M, N] W[N, K] on dr_kn_kernel (gd_dr_kn_splits / gd_dr_kn_launch: 80 x 128 tiles, one
    (split, tile) task per wave slot, at least eight chunks of 16 per split, an even number of chunks per split), or None when
    the kernel does not take the shape.  The kernel writes `splits` slabs of M x round4(K) floats; gdmcf_linear_ws_bytes sizes the
    workspace for the `asked` >= splits slabs of gd_dr_kn_splits, before the chunks per split were rounded up."""
    if M < 16 or K < 64 or N < 4096:
        return None
    tm, tn = cdiv(M, 80), cdiv(K, 128)
    if tm * 80 * 100 > M * 112 or tn * 128 * 100 > K * 112 or tm * tn > 4 * n_cu:
        return None
    chunks = cdiv(N, 16)
    splits = min(4 * n_cu // (tm * tn), chunks // 8)
    if splits > 64:
        splits = 64
    if splits < 2:
        return None
    cps = (cdiv(chunks, splits) + 1) & ~1
    return cdiv(chunks, cps), cps, splits
