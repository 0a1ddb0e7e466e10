// The BPR objective of LightGCN training (reference lightGCN.py:207-251, :287-300) without autograd: the triple sampler, the
// loss with its per-triple derivative, and the scatter of that derivative into the cotangent of the propagated table.
//
// All three are latency / launch bound, not bandwidth bound: a batch of 1024 triples touches ~3 k rows of 256 bytes (d = 64).
// The lane mapping is the short-row mapping of the SpMM: a row of d floats is served by a group of LG = 2^ceil(log2(d/4)) lanes
// (capped at 64) that hold one float4 each -- 16 lanes at d = 64, four triples (or scatter entries) to a wave -- and a dot
// product is reduced inside the group by xor shuffles.  d % 4 != 0 (or unaligned rows) takes the same kernels with element-wise
// loads and stores.
//
// gdmcf_bpr_sample_pool_f32 generalises the reference's per-user draw (lightGCN.py:225-246: one positive, one negative) to
// n_negs negatives per positive, each the best-scored of `pool` uniform candidates under the current propagated table
// (dynamic negative sampling); n_negs = pool = 1 is gdmcf_bpr_sample_f32's draw bit for bit.  It gathers B n_negs (1 + pool)
// rows and is latency bound like the rest: a lane group per slot, the next candidate's row in flight over each reduction.
//
// Nothing here uses a float atomic: the loss is reduced from per-triple partials in one fixed order, and the scatter gives every
// destination row ONE writer that adds the row's contributions in sorted order (gdmcf_bpr_grad_f32), so results are the same
// bits in every run whatever ids repeat.
#include <math.h>

#include "draws.h"

namespace {

template <bool VEC>
__device__ __forceinline__ f32x4 bpr_load4(const float* __restrict__ row, int c0, int d) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        if (c0 < d) v = *reinterpret_cast<const f32x4*>(row + c0);
    } else {
        if (c0 < d) v.x = row[c0];
        if (c0 + 1 < d) v.y = row[c0 + 1];
        if (c0 + 2 < d) v.z = row[c0 + 2];
        if (c0 + 3 < d) v.w = row[c0 + 3];
    }
    return v;
}

template <bool VEC>
__device__ __forceinline__ void bpr_store4(float* __restrict__ row, int c0, int d, f32x4 v) {
    if (VEC) {
        if (c0 < d) *reinterpret_cast<f32x4*>(row + c0) = v;
    } else {
        if (c0 < d) row[c0] = v.x;
        if (c0 + 1 < d) row[c0 + 1] = v.y;
        if (c0 + 2 < d) row[c0 + 2] = v.z;
        if (c0 + 3 < d) row[c0 + 3] = v.w;
    }
}

// the n-sided die from one 32-bit word: floor(w n / 2^32) (bias <= n / 2^32)
__device__ __forceinline__ uint32_t bpr_mulhi(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * (uint64_t)n) >> 32); }

// ---------------------------------------------------------------------------------------------
// (a) sampler: one thread per triple
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bpr_sample_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                          const int64_t* __restrict__ users, int B, int n_users, int n_items,
                                                          uint64_t seed, uint64_t offset, int64_t* __restrict__ pos,
                                                          int64_t* __restrict__ neg, int32_t* __restrict__ flag) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= B) return;
    const int64_t u = users[j];
    int64_t beg = 0, deg = 0;
    if (u >= 0 && u < n_users) {
        beg = indptr[u];
        deg = indptr[u + 1] - beg;
    }
    if (deg <= 0 || deg >= n_items) {  // nothing to draw a positive (or a negative) from
        pos[j] = -1;
        neg[j] = -1;
        if (flag) *flag = 1;
        return;
    }
    const uint4 w = gd_philox_block((uint32_t)j, 0, GD_STREAM_BPR, offset, gd_philox_key(seed));
    const int32_t* __restrict__ row = indices + beg;
    pos[j] = row[bpr_mulhi(w.x, (uint32_t)deg)];
    // the r-th item (from 0) that is NOT in the sorted row: row[i] - i items are missing below row[i], so with i the first
    // position where that count exceeds r (i = deg: none does) exactly i row entries lie below the answer r + i
    const int r = (int)bpr_mulhi(w.y, (uint32_t)(n_items - (int)deg));
    int lo = 0, hi = (int)deg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] - mid > r) hi = mid; else lo = mid + 1;
    }
    neg[j] = r + lo;
}

// ---------------------------------------------------------------------------------------------
// (a') sampler with n_negs negatives per positive, each the best of a pool of candidates: one lane group per slot (j, k)
// ---------------------------------------------------------------------------------------------
// the word of candidate q of triple j (draws.h, GD_STREAM_BPR): q < 3 is word y, z, w of block 0 (word x draws the positive),
// q >= 3 word (q - 3) % 4 of block 1 + (q - 3) / 4.  `first` receives word x of the block the candidate came from.
__device__ __forceinline__ uint32_t bpr_candidate_word(int j, int q, uint64_t seed, uint64_t offset, uint32_t& first) {
    const int blk = q < 3 ? 0 : 1 + ((q - 3) >> 2), word = q < 3 ? q + 1 : (q - 3) & 3;
    const uint4 w = gd_philox_block((uint32_t)j, blk, GD_STREAM_BPR, offset, gd_philox_key(seed));
    first = w.x;
    return word == 0 ? w.x : word == 1 ? w.y : word == 2 ? w.z : w.w;
}

// the r-th item (from 0) that is NOT in the sorted row: bpr_sample_kernel's search
__device__ __forceinline__ int bpr_nth_missing(const int32_t* __restrict__ row, int deg, int r) {
    int lo = 0, hi = deg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (row[mid] - mid > r) hi = mid; else lo = mid + 1;
    }
    return r + lo;
}

__device__ __forceinline__ float bpr_dot4(const f32x4& a, const f32x4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// Slot s = j * n_negs + k.  Lane l of the group draws and searches candidates c = l, l + LG, ... of the slot's pool (number
// q = k * pool + c of the triple), then the group walks LG candidates at a time by shuffle: one item row against the user row
// (one float4 per lane, held in registers), the row of the next candidate loaded before the current one is reduced.  Every lane
// holds the same score after the xor reduction, so all keep the same best; lane 0 stores.  pool == 1 is launched with LG = 1 and
// M == nullptr: the one candidate is the negative and nothing is scored.
template <bool VEC>
__global__ __launch_bounds__(256) void bpr_sample_pool_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                               const int64_t* __restrict__ users, int B, int n_negs, int pool,
                                                               int n_users, int n_items, const float* __restrict__ M, int64_t ldm,
                                                               int d, int LG, uint64_t seed, uint64_t offset,
                                                               int64_t* __restrict__ pos, int64_t* __restrict__ neg,
                                                               int32_t* __restrict__ flag) {
    const int tid = threadIdx.x;
    const int g = tid / LG, l = tid - g * LG;
    const int64_t s = (int64_t)blockIdx.x * (256 / LG) + g;
    if (s >= (int64_t)B * n_negs) return;  // (whole groups leave: the shuffles below stay inside a group)
    const int j = (int)(s / n_negs), k = (int)(s - (int64_t)j * n_negs);
    const int64_t u = users[j];
    int64_t beg = 0, deg64 = 0;
    if (u >= 0 && u < n_users) {
        beg = indptr[u];
        deg64 = indptr[u + 1] - beg;
    }
    if (deg64 <= 0 || deg64 >= n_items) {  // nothing to draw a positive (or a negative) from
        if (l == 0) {
            if (k == 0) pos[j] = -1;
            neg[s] = -1;
            if (flag) *flag = 1;
        }
        return;
    }
    const int deg = (int)deg64;
    const int32_t* __restrict__ row = indices + beg;
    const bool score = M != nullptr && pool > 1;
    const int ncc = (d + 4 * LG - 1) / (4 * LG);  // column passes (1 up to d = 256): the same count in every lane
    const float* __restrict__ mu = score ? M + u * ldm : nullptr;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f};
    if (score) a0 = bpr_load4<VEC>(mu, 4 * l, d);  // the user row: once per slot
    int best = 0;
    float best_score = 0.f;
    for (int cb = 0; cb < pool; cb += LG) {
        const int c = cb + l;
        int cand = 0;
        if (c < pool) {
            uint32_t first;
            const uint32_t w = bpr_candidate_word(j, k * pool + c, seed, offset, first);
            cand = bpr_nth_missing(row, deg, (int)bpr_mulhi(w, (uint32_t)(n_items - deg)));
            if (k == 0 && c == 0) pos[j] = row[bpr_mulhi(first, (uint32_t)deg)];  // (candidate 0 of the triple lives in block 0)
        }
        if (!score) {  // pool == 1 (LG = 1): the candidate is the negative
            best = cand;
            break;
        }
        const int nv = min(LG, pool - cb);
        int ci = __shfl(cand, 0, LG);
        f32x4 b = bpr_load4<VEC>(M + ((int64_t)n_users + ci) * ldm, 4 * l, d);
        for (int i = 0; i < nv; ++i) {
            const int cn = __shfl(cand, min(i + 1, nv - 1), LG);
            const float* __restrict__ mi = M + ((int64_t)n_users + ci) * ldm;
            f32x4 bn = b;
            if (i + 1 < nv) bn = bpr_load4<VEC>(M + ((int64_t)n_users + cn) * ldm, 4 * l, d);  // in flight over the reduction
            float sc = bpr_dot4(a0, b);
            for (int cc = 1; cc < ncc; ++cc) {
                const int c0 = 4 * (l + cc * LG);
                sc += bpr_dot4(bpr_load4<VEC>(mu, c0, d), bpr_load4<VEC>(mi, c0, d));
            }
            for (int m = LG >> 1; m > 0; m >>= 1) sc += __shfl_xor(sc, m);  // (groups are aligned: lane ^ m stays inside)
            // the first candidate is kept; a later one replaces it only with a strictly greater score (never with a NaN)
            if ((cb == 0 && i == 0) || sc > best_score) {
                best = ci;
                best_score = sc;
            }
            ci = cn;
            b = bn;
        }
    }
    if (l == 0) neg[s] = best;
}

// ---------------------------------------------------------------------------------------------
// (b) loss: one lane group per triple, then one fixed-order reduction
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void bpr_loss_kernel(const float* __restrict__ M, int64_t ldm, const float* __restrict__ E0,
                                                        int64_t lde, int d, int LG, const int64_t* __restrict__ users,
                                                        const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, int B,
                                                        int n_users, int n_items, float* __restrict__ coef, float* __restrict__ ws,
                                                        int32_t* __restrict__ flag) {
    const int tid = threadIdx.x;
    const int g = tid / LG, l = tid - g * LG;
    const int j = blockIdx.x * (256 / LG) + g;
    const bool live = j < B;  // (no early exit: every lane takes part in the shuffles)
    int64_t u = 0, p = 0, n = 0;
    bool ok = false;
    if (live) {
        u = users[j];
        p = pos[j];
        n = neg[j];
        ok = u >= 0 && u < n_users && p >= 0 && p < n_items && n >= 0 && n < n_items;
    }
    if (!ok) u = p = n = 0;  // an id out of range: flagged below, contributes nothing, reads row 0
    const float* __restrict__ mu = M + u * ldm;
    const float* __restrict__ mp = M + (n_users + p) * ldm;
    const float* __restrict__ mn = M + (n_users + n) * ldm;
    const float* __restrict__ eu = E0 + u * lde;
    const float* __restrict__ ep = E0 + (n_users + p) * lde;
    const float* __restrict__ en = E0 + (n_users + n) * lde;
    float sp = 0.f, sn = 0.f, rg = 0.f;
    for (int c0 = 4 * l; c0 < d; c0 += 4 * LG) {
        const f32x4 a = bpr_load4<VEC>(mu, c0, d), b = bpr_load4<VEC>(mp, c0, d), c = bpr_load4<VEC>(mn, c0, d);
        const f32x4 x = bpr_load4<VEC>(eu, c0, d), y = bpr_load4<VEC>(ep, c0, d), z = bpr_load4<VEC>(en, c0, d);
        sp += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        sn += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
        rg += (x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w) + (y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w) +
              (z.x * z.x + z.y * z.y + z.z * z.z + z.w * z.w);
    }
    for (int m = LG >> 1; m > 0; m >>= 1) {  // (groups are aligned: lane ^ m stays inside)
        sp += __shfl_xor(sp, m);
        sn += __shfl_xor(sn, m);
        rg += __shfl_xor(rg, m);
    }
    if (l == 0 && live) {
        const float x = sn - sp;
        // torch.nn.functional.softplus (beta 1, threshold 20) and its derivative, z / (z + 1) with z = exp(x)
        const float z = expf(fminf(x, 20.f));
        float soft = x > 20.f ? x : log1pf(z);
        float sig = x > 20.f ? 1.f : z / (z + 1.f);
        if (!ok) {
            soft = sig = rg = 0.f;
            if (flag) *flag = 1;
        }
        coef[j] = sig / (float)B;
        ws[j] = soft;
        ws[B + j] = rg;
    }
}

// mf = mean_j ws[j], reg = 0.5 sum_j ws[B + j] / B: thread t adds j = t, t + 256, ... in this order, then a fixed LDS tree
__global__ __launch_bounds__(256) void bpr_reduce_kernel(const float* __restrict__ ws, int B, float* __restrict__ mf,
                                                          float* __restrict__ reg) {
    __shared__ float s0[256], s1[256];
    const int tid = threadIdx.x;
    float a = 0.f, b = 0.f;
    for (int j = tid; j < B; j += 256) {
        a += ws[j];
        b += ws[B + j];
    }
    s0[tid] = a;
    s1[tid] = b;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (tid < m) {
            s0[tid] += s0[tid + m];
            s1[tid] += s1[tid + m];
        }
        __syncthreads();
    }
    if (tid == 0) {
        *mf = s0[0] / (float)B;
        *reg = 0.5f * s1[0] / (float)B;
    }
}

// ---------------------------------------------------------------------------------------------
// (c) scatter without atomics: entry e of the batch = (role e / B, triple e % B); `order` lists the 3B entries by node
// ---------------------------------------------------------------------------------------------
struct BprIds {
    const int64_t* users;
    const int64_t* pos;
    const int64_t* neg;
    int B, n_users, n_items;
};

// node of an entry, -1 when its id is out of range (gdmcf_bpr_loss_f32 has flagged it; it gets no row)
__device__ __forceinline__ int64_t bpr_node(const BprIds& t, int e) {
    e = min(max(e, 0), 3 * t.B - 1);
    const int role = e / t.B, j = e - role * t.B;
    if (role == 0) {
        const int64_t u = t.users[j];
        return (u >= 0 && u < t.n_users) ? u : -1;
    }
    const int64_t i = role == 1 ? t.pos[j] : t.neg[j];
    return (i >= 0 && i < t.n_items) ? t.n_users + i : -1;
}

template <bool VEC>
__global__ __launch_bounds__(256) void bpr_grad_kernel(int mode, const int32_t* __restrict__ order, BprIds t,
                                                        const float* __restrict__ coef, const float* __restrict__ src, int64_t lds_,
                                                        int d, int LG, float* __restrict__ out, int64_t ldo, float scale,
                                                        float* __restrict__ zero_rows, int64_t ldz) {
    const int tid = threadIdx.x;
    const int g = tid / LG, l = tid - g * LG;
    const int k = blockIdx.x * (256 / LG) + g;
    const int n3 = 3 * t.B;
    if (k >= n3) return;  // (whole groups leave: the shuffles below stay inside a group)
    const int64_t node = bpr_node(t, order[k]);
    if (node < 0) return;
    if (k > 0 && bpr_node(t, order[k - 1]) == node) return;  // the run's first entry is its only writer
    const int gshift = (tid & 63) & ~(LG - 1);  // first lane of the group inside its wave
    const unsigned long long gmask = LG == 64 ? ~0ull : ((1ull << LG) - 1ull);
    const int ncc = (d + 4 * LG - 1) / (4 * LG);  // column passes (1 up to d = 256): the same count in every lane

    if (mode == 1) {
        // the regulariser's rows: out[node] += scale * multiplicity * src[node]   (src = E0, scale = decay / B)
        int mult = 0;
        for (int kb = k;; kb += LG) {
            const int kk = kb + l;
            const bool mine = kk < n3 && bpr_node(t, order[kk]) == node;
            const unsigned long long bits = (__ballot(mine) >> gshift) & gmask;
            const int nv = ~bits ? __builtin_ctzll(~bits) : 64;  // (entries of a run are consecutive: the leading ones)
            mult += nv;
            if (nv < LG) break;
        }
        const float s = scale * (float)mult;
        for (int cc = 0; cc < ncc; ++cc) {
            const int c0 = 4 * (l + cc * LG);
            const f32x4 e = bpr_load4<VEC>(src + node * lds_, c0, d);
            f32x4 o = bpr_load4<VEC>(out + node * ldo, c0, d);
            o.x += s * e.x; o.y += s * e.y; o.z += s * e.z; o.w += s * e.w;
            bpr_store4<VEC>(out + node * ldo, c0, d, o);
            if (zero_rows) bpr_store4<VEC>(zero_rows + node * ldz, c0, d, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        return;
    }

    // mode 0: out[node] = sum over the run, in sorted order, of   user: coef_j (src[neg_j] - src[pos_j]),
    // pos: -coef_j src[u_j],  neg: +coef_j src[u_j]   (src = M).  The group reads LG entries' ids at once (lane l: entry kb + l),
    // then walks them by shuffle, so a run costs one round of dependent id loads per LG entries, not one per entry.
    for (int cc = 0; cc < ncc; ++cc) {
        const int c0 = 4 * (l + cc * LG);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kb = k;; kb += LG) {
            const int kk = kb + l;
            bool mine = false;
            float w = 0.f;
            int ra = 0, rb = -1;
            if (kk < n3) {
                const int e = min(max(order[kk], 0), n3 - 1);
                if (bpr_node(t, e) == node) {
                    mine = true;
                    const int role = e / t.B, j = e - role * t.B;
                    const float c = coef[j];
                    // (the other ids of the triple are clamped for the READ only; a triple with a bad id has coef 0)
                    const int64_t u = min(max(t.users[j], (int64_t)0), (int64_t)t.n_users - 1);
                    if (role == 0) {
                        w = c;
                        ra = (int)(t.n_users + min(max(t.neg[j], (int64_t)0), (int64_t)t.n_items - 1));
                        rb = (int)(t.n_users + min(max(t.pos[j], (int64_t)0), (int64_t)t.n_items - 1));
                    } else {
                        w = role == 1 ? -c : c;
                        ra = (int)u;
                    }
                }
            }
            const unsigned long long bits = (__ballot(mine) >> gshift) & gmask;
            const int nv = ~bits ? __builtin_ctzll(~bits) : 64;
            for (int i = 0; i < nv; ++i) {
                const float wi = __shfl(w, i, LG);
                const int ai = __shfl(ra, i, LG), bi = __shfl(rb, i, LG);
                f32x4 a = bpr_load4<VEC>(src + (int64_t)ai * lds_, c0, d);
                if (bi >= 0) {
                    const f32x4 b = bpr_load4<VEC>(src + (int64_t)bi * lds_, c0, d);
                    a.x -= b.x; a.y -= b.y; a.z -= b.z; a.w -= b.w;
                }
                acc.x += wi * a.x; acc.y += wi * a.y; acc.z += wi * a.z; acc.w += wi * a.w;
            }
            if (nv < LG) break;
        }
        bpr_store4<VEC>(out + node * ldo, c0, d, acc);
    }
}

int bpr_lane_group(int d) {
    const int chunks = (d + 3) / 4;
    int lg = 1;
    while (lg < chunks && lg < 64) lg <<= 1;
    return lg;
}

}  // namespace

extern "C" {

int gdmcf_bpr_sample_f32(const int64_t* indptr, const int32_t* indices, const int64_t* users, int B, int n_users, int n_items,
                         uint64_t seed, uint64_t offset, int64_t* pos, int64_t* neg, int32_t* flag, void* stream) {
    GD_CHECK_SHAPE(B > 0 && n_users > 0 && n_items > 0, "bpr_sample: bad shape");
    GD_CHECK_OFFSET(offset, "bpr_sample");
    GD_CHECK_ARG(indptr && indices && users && pos && neg, "bpr_sample: null pointer");
    hipLaunchKernelGGL(bpr_sample_kernel, dim3(gd_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, indptr, indices, users, B,
                       n_users, n_items, seed, offset, pos, neg, flag);
    return gd_launch_status("bpr_sample");
}

int gdmcf_bpr_sample_pool_f32(const int64_t* indptr, const int32_t* indices, const int64_t* users, int B, int n_negs, int pool,
                              int n_users, int n_items, const float* M, int64_t ldm, int d, uint64_t seed, uint64_t offset,
                              int64_t* pos, int64_t* neg, int32_t* flag, void* stream) {
    GD_CHECK_SHAPE(B > 0 && n_negs > 0 && pool > 0 && n_users > 0 && n_items > 0, "bpr_sample_pool: bad shape");
    GD_CHECK_SHAPE((int64_t)n_negs * pool < (1 << 20), "bpr_sample_pool: n_negs * pool must stay below 2^20");
    GD_CHECK_SHAPE(M == nullptr || (d >= 1 && ldm >= d), "bpr_sample_pool: bad table shape");
    GD_CHECK_OFFSET(offset, "bpr_sample_pool");
    GD_CHECK_ARG(indptr && indices && users && pos && neg, "bpr_sample_pool: null pointer");
    GD_CHECK_ARG(M != nullptr || pool == 1, "bpr_sample_pool: a pool of candidates needs the propagated table");
    const bool scored = pool > 1;
    const int LG = scored ? bpr_lane_group(d) : 1;  // nothing to score: one thread per slot
    GD_CHECK_SHAPE((int64_t)B * n_negs * LG < 2147483647LL && (int64_t)n_users + n_items < 2147483647LL,
                   "bpr_sample_pool: batch or table too large");
    const bool vec = scored && d % 4 == 0 && ldm % 4 == 0 && gd_aligned16(M);
    const dim3 grid((unsigned)(((int64_t)B * n_negs + 256 / LG - 1) / (256 / LG)));
    const float* table = scored ? M : nullptr;
    if (vec)
        hipLaunchKernelGGL(bpr_sample_pool_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, indptr, indices, users, B, n_negs,
                           pool, n_users, n_items, table, ldm, d, LG, seed, offset, pos, neg, flag);
    else
        hipLaunchKernelGGL(bpr_sample_pool_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, indptr, indices, users, B, n_negs,
                           pool, n_users, n_items, table, ldm, d, LG, seed, offset, pos, neg, flag);
    return gd_launch_status("bpr_sample_pool");
}

int gdmcf_bpr_loss_f32(const float* M, int64_t ldm, const float* E0, int64_t lde, int d, const int64_t* users, const int64_t* pos,
                       const int64_t* neg, int B, int n_users, int n_items, float* coef, float* ws, float* mf, float* reg,
                       int32_t* flag, void* stream) {
    GD_CHECK_SHAPE(B > 0 && n_users > 0 && n_items > 0 && d >= 1 && ldm >= d && lde >= d, "bpr_loss: bad shape");
    GD_CHECK_ARG(M && E0 && users && pos && neg && coef && ws && mf && reg, "bpr_loss: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const int LG = bpr_lane_group(d);
    const bool vec = d % 4 == 0 && ldm % 4 == 0 && lde % 4 == 0 && gd_aligned16(M) && gd_aligned16(E0);
    const dim3 grid(gd_cdiv(B, 256 / LG));
    if (vec)
        hipLaunchKernelGGL(bpr_loss_kernel<true>, grid, dim3(256), 0, s, M, ldm, E0, lde, d, LG, users, pos, neg, B, n_users, n_items,
                           coef, ws, flag);
    else
        hipLaunchKernelGGL(bpr_loss_kernel<false>, grid, dim3(256), 0, s, M, ldm, E0, lde, d, LG, users, pos, neg, B, n_users,
                           n_items, coef, ws, flag);
    hipLaunchKernelGGL(bpr_reduce_kernel, dim3(1), dim3(256), 0, s, ws, B, mf, reg);
    return gd_launch_status("bpr_loss");
}

int gdmcf_bpr_grad_f32(int mode, const int32_t* order, const int64_t* users, const int64_t* pos, const int64_t* neg, int B,
                       int n_users, int n_items, const float* coef, const float* src, int64_t ld_src, int d, float* out,
                       int64_t ld_out, float scale, float* zero_rows, int64_t ld_zero, void* stream) {
    GD_CHECK_SHAPE(B > 0 && n_users > 0 && n_items > 0 && d >= 1 && ld_src >= d && ld_out >= d, "bpr_grad: bad shape");
    GD_CHECK_SHAPE((int64_t)B * 3 < 2147483647LL && (int64_t)n_users + n_items < 2147483647LL, "bpr_grad: batch or table too large");
    GD_CHECK_ARG(mode == 0 || mode == 1, "bpr_grad: mode must be 0 (cotangent) or 1 (regulariser rows)");
    GD_CHECK_ARG(order && users && pos && neg && src && out && (mode == 1 || coef), "bpr_grad: null pointer");
    GD_CHECK_ARG(zero_rows == nullptr || (mode == 1 && ld_zero >= d), "bpr_grad: zero_rows goes with mode 1");
    const int LG = bpr_lane_group(d);
    const bool vec = d % 4 == 0 && ld_src % 4 == 0 && ld_out % 4 == 0 && gd_aligned16(src) && gd_aligned16(out) &&
                     (zero_rows == nullptr || (ld_zero % 4 == 0 && gd_aligned16(zero_rows)));
    const BprIds t{users, pos, neg, B, n_users, n_items};
    const dim3 grid(gd_cdiv(3 * B, 256 / LG));
    if (vec)
        hipLaunchKernelGGL(bpr_grad_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, mode, order, t, coef, src, ld_src, d, LG, out,
                           ld_out, scale, zero_rows, ld_zero);
    else
        hipLaunchKernelGGL(bpr_grad_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, mode, order, t, coef, src, ld_src, d, LG,
                           out, ld_out, scale, zero_rows, ld_zero);
    return gd_launch_status("bpr_grad");
}

}  // extern "C"
