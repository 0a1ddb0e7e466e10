// Fused score product + masked top-k (reference lightGCN.py:67-127, get_metrics: user_emb @ item_emb.T, -inf on the training
// interactions, torch.topk): the [n_rows, n_items] score matrix exists only as MFMA accumulators.
//
// A 256-thread workgroup owns a tile of 16 RB user rows and a range of items.  Its four waves share the rows and split the
// items: per step wave w multiplies the tile by items base + 16 w .. + 15 (v_mfma_f32_16x16x4_f32; the user fragments stay in
// registers when d <= 64, otherwise they are re-read through L1/L2 in every step), so a lane ends up with the scores of ONE item
// for 4 RB rows.  Each score is compared with its row's running bound -- a lower bound of the row's k-th best (key, ~index) pair
// that only rises -- and the few survivors are looked up in the history bitmap (LDS, rebuilt from the CSR mask every BM_ITEMS
// items), get the key of -inf when masked (gdmcf_topk_masked_f32's convention: masked items rank last, lowest index first) and
// are appended to the row's candidate list in LDS.  A step appends at most 64 pairs per row; when a list could overflow in the
// next step all lists are sorted (bitonic, descending), cut to k and the bounds are raised to the k-th pair.  The appends go
// through LDS atomics, so the ORDER inside a list varies, but which pairs are in it does not, and pairs are unique: the sorted
// result is the same bits in every run.
// When there are too few row tiles to fill the chip the items are split into slabs: each (tile, slab) workgroup writes its k
// best pairs to the workspace and score_merge_kernel sorts a row's slabs together.
#include "common.h"
#include "score_product.h"

namespace {

__device__ __forceinline__ uint32_t st_order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float st_key_to_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}
constexpr uint32_t ST_NEG_INF_KEY = 0x007FFFFFu;  // st_order_key(-inf)
constexpr int ST_BM_ITEMS = 2048;                  // items covered by one build of the history bitmap
constexpr int ST_BM_WORDS = ST_BM_ITEMS / 32;
constexpr int ST_STEP = SP_STEP;                   // items per workgroup step (4 waves x 16)
typedef unsigned long long u64;

// all lists of the tile: pad to CAP with 0 (below every real pair), bitonic sort descending, cut to k, raise the bounds
__device__ void st_compact(u64* cand, uint32_t* cnt, u64* thr, int R, int CAP, int k, int tid) {
    for (int e = tid; e < R * CAP; e += 256) {
        const int r = e / CAP, j = e - r * CAP;
        if (j >= (int)cnt[r]) cand[e] = 0ull;
    }
    __syncthreads();
    const int half = CAP >> 1;
    for (int size = 2; size <= CAP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < R * half; e += 256) {
                const int r = e / half, j = e - r * half;
                const int lo = ((j / stride) * stride * 2) + (j % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                u64* c = cand + (size_t)r * CAP;
                const u64 a = c[lo], b = c[hi];
                if ((a < b) == desc) {
                    c[lo] = b;
                    c[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    if (tid < R) {
        const int n = (int)cnt[tid];
        if (n >= k) {
            cnt[tid] = (uint32_t)k;
            thr[tid] = cand[(size_t)tid * CAP + k - 1];
        }
    }
    __syncthreads();
}

template <int RB, bool AREG>
__global__ __launch_bounds__(256) void score_topk_kernel(const float* __restrict__ U, int64_t ldu, const int64_t* __restrict__ uid,
                                                          int n_rows, const float* __restrict__ V, int64_t ldi, int n_items, int d,
                                                          const int64_t* __restrict__ mptr, const int32_t* __restrict__ midx, int k,
                                                          int R, int CAP, int nslab, int slab_items, int vec,
                                                          int64_t* __restrict__ out_idx, float* __restrict__ out_val,
                                                          u64* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* cand = reinterpret_cast<u64*>(smem_raw);           // [R][CAP]
    u64* thr = cand + (size_t)R * CAP;                       // [R]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(thr + R);    // [R]
    uint32_t* bitmap = cnt + R;                              // [R][ST_BM_WORDS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x / nslab, slab = blockIdx.x - tile * nslab;
    const int row0 = tile * R;
    const int rows_here = min(R, n_rows - row0);
    const int i0 = slab * slab_items, i1 = min(n_items, i0 + slab_items);
    const int lc = lane & 15, lg = lane >> 4;

    if (tid < R) {
        cnt[tid] = 0u;
        thr[tid] = 0ull;
    }
    // the tile's rows of the user table (rows past the end repeat the last one and are never selected from)
    const float* arow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = row0 + min(rb * 16 + lc, rows_here - 1);
        arow[rb] = U + (uid ? uid[r] : (int64_t)r) * ldu;
    }
    f32x4 areg[RB][4];  // (the product step -- fragments, k order -- is score_product.h's, shared with score_rank.hip)
    if constexpr (AREG) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) sp_load_frags(areg[rb], arow[rb], lg, d, vec != 0);
    }
    float thrf[RB][4];  // the bounds of this lane's rows as floats: -inf = everything passes, +inf (rows past the end) = nothing
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int q = 0; q < 4; ++q) thrf[rb][q] = (rb * 16 + 4 * lg + q < rows_here) ? -INFINITY : INFINITY;

    auto item_row = [&](int base) -> const float* { return V + (int64_t)min(base + 16 * wave + lc, n_items - 1) * ldi; };
    f32x4 bcur[4], bnext[4];
    if constexpr (AREG) sp_load_frags(bcur, item_row(i0), lg, d, vec != 0);

    for (int cbase = i0; cbase < i1; cbase += ST_BM_ITEMS) {
        // ---- history bitmap of items cbase .. cbase + ST_BM_ITEMS - 1 ----
        __syncthreads();
        for (int e = tid; e < R * ST_BM_WORDS; e += 256) bitmap[e] = 0u;
        __syncthreads();
        if (mptr) {
            for (int r = wave; r < rows_here; r += 4) {
                const int64_t beg = mptr[row0 + r], end = mptr[row0 + r + 1];
                for (int64_t j = beg + lane; j < end; j += 64) {
                    const int c = midx[j] - cbase;
                    if (c >= 0 && c < ST_BM_ITEMS) atomicOr(&bitmap[r * ST_BM_WORDS + (c >> 5)], 1u << (c & 31));
                }
            }
        }
        __syncthreads();
        const int cend = min(i1, cbase + ST_BM_ITEMS);
        for (int base = cbase; base < cend; base += ST_STEP) {
            f32x4 acc[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (AREG) {
                // the next step's items are requested before this step's products (addresses clamped to the table)
                sp_load_frags(bnext, item_row(base + ST_STEP), lg, d, vec != 0);
                sp_mfma_frags<RB>(acc, areg, bcur, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) bcur[j] = bnext[j];
            } else {
                sp_mfma_reread<RB>(acc, arow, item_row(base), lg, d, vec != 0);
            }
            // ---- selection: acc[rb][q] = score(row rb*16 + 4*lg + q, item base + 16*wave + lc) ----
            bool pass = false;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int q = 0; q < 4; ++q) pass = pass || !(acc[rb][q] < thrf[rb][q]);
            const int item = base + 16 * wave + lc;
            if (pass && item < i1) {
                const int bi = item - cbase;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = rb * 16 + 4 * lg + q;
                        if (!(acc[rb][q] < thrf[rb][q]) && r < rows_here) {
                            uint32_t key = st_order_key(acc[rb][q]);
                            if (bitmap[r * ST_BM_WORDS + (bi >> 5)] & (1u << (bi & 31))) key = ST_NEG_INF_KEY;
                            const u64 pair = ((u64)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)item);
                            if (pair > thr[r]) {
                                const uint32_t slot = atomicAdd(&cnt[r], 1u);
                                if (slot < (uint32_t)CAP) cand[(size_t)r * CAP + slot] = pair;
                            }
                        }
                    }
            }
            // ---- a list that could overflow in the next step?  sort, cut, raise the bounds ----
            // (the counters are read only after EVERY wave's appends of this step: __syncthreads_or evaluates its argument
            // before its own barrier, and a count read early could be 48 short and let the next step overflow the list)
            __syncthreads();
            const int full = __syncthreads_or((tid < R) && ((int)cnt[tid] > CAP - ST_STEP));
            if (full) {
                st_compact(cand, cnt, thr, R, CAP, k, tid);
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int r = rb * 16 + 4 * lg + q;
                        if (r < rows_here) {
                            const u64 t = thr[r];
                            thrf[rb][q] = t ? st_key_to_float((uint32_t)(t >> 32)) : -INFINITY;
                        }
                    }
            }
        }
    }
    __syncthreads();
    st_compact(cand, cnt, thr, R, CAP, k, tid);
    // the first min(k, items of the slab) pairs of every list are its answer (the rest of the k slots: 0, below every pair)
    for (int e = tid; e < rows_here * k; e += 256) {
        const int r = e / k, j = e - r * k;
        const u64 c = j < (int)cnt[r] ? cand[(size_t)r * CAP + j] : 0ull;
        if (nslab > 1) {
            ws[((int64_t)(row0 + r) * nslab + slab) * k + j] = c;
        } else {
            out_idx[(int64_t)(row0 + r) * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull));
            if (out_val) out_val[(int64_t)(row0 + r) * k + j] = st_key_to_float((uint32_t)(c >> 32));
        }
    }
}

// one workgroup per row: the nslab * k pairs of its slabs sorted together, the first k are the row's answer
__global__ __launch_bounds__(256) void score_merge_kernel(const u64* __restrict__ ws, int n, int NP, int k,
                                                           int64_t* __restrict__ out_idx, float* __restrict__ out_val) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64* c = reinterpret_cast<u64*>(smem_raw);  // [NP]
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    for (int j = tid; j < NP; j += 256) c[j] = j < n ? ws[row * n + j] : 0ull;
    __syncthreads();
    for (int size = 2; size <= NP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int j = tid; j < NP / 2; j += 256) {
                const int lo = ((j / stride) * stride * 2) + (j % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const u64 a = c[lo], b = c[hi];
                if ((a < b) == desc) {
                    c[lo] = b;
                    c[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += 256) {
        const u64 p = c[j];
        out_idx[row * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(p & 0xFFFFFFFFull));
        if (out_val) out_val[row * k + j] = st_key_to_float((uint32_t)(p >> 32));
    }
}

struct StPlan {
    int RB, R, CAP, nslab, slab_items;
};

// Tile height and list capacity by k (a list must hold k pairs plus one step's 64 appends; 16 RB rows x CAP pairs <= 128 KiB),
// and the item slabs: enough workgroups for two per CU, slabs of whole steps holding at least k items, and a workspace of at
// most 5 % of the score matrix it stands in for (8 k nslab bytes per row against 4 n_items).
StPlan st_plan(int n_rows, int n_items, int k) {
    StPlan p;
    if (k <= 160) { p.RB = 4; p.R = 64; p.CAP = 256; }
    else if (k <= 416) { p.RB = 2; p.R = 32; p.CAP = 512; }
    else { p.RB = 1; p.R = 8; p.CAP = 2048; }  // (half of the 16-row block is computed and ignored)
    const int tiles = gd_cdiv(n_rows, p.R);
    int want = tiles >= 256 ? 1 : gd_cdiv(512, tiles);
    const int64_t by_ws = (int64_t)n_items / (40 * (int64_t)k);
    const int64_t by_len = (int64_t)n_items / (int64_t)(k > 512 ? k : 512);
    if (want > 16) want = 16;
    if (want > by_ws) want = (int)by_ws;
    if (want > by_len) want = (int)by_len;
    if (want < 1) want = 1;
    p.slab_items = gd_cdiv(gd_cdiv(n_items, want), ST_STEP) * ST_STEP;
    p.nslab = gd_cdiv(n_items, p.slab_items);
    return p;
}

}  // namespace

extern "C" {

size_t gdmcf_score_topk_ws_bytes(int n_rows, int n_items, int d, int k) {
    (void)d;
    if (n_rows <= 0 || n_items <= 0 || k < 1 || k > n_items || k > 1024) return 0;
    const StPlan p = st_plan(n_rows, n_items, k);
    return p.nslab > 1 ? (size_t)n_rows * p.nslab * k * sizeof(u64) : 0;
}

int gdmcf_score_topk_f32(const float* user_emb, int64_t ldu, const int64_t* user_ids, int n_rows, const float* item_emb,
                         int64_t ldi, int n_items, int d, const int64_t* mask_indptr, const int32_t* mask_indices, int k,
                         int64_t* out_idx, float* out_val, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_SHAPE(n_rows > 0 && n_items > 0 && d >= 1 && ldu >= d && ldi >= d, "score_topk: bad shape");
    GD_CHECK_SHAPE(k >= 1 && k <= n_items, "score_topk: k out of range (selected index k out of range)");
    GD_CHECK_ARG(k <= 1024, "score_topk: k > 1024 unsupported");
    GD_CHECK_ARG(d <= 4096, "score_topk: d > 4096 unsupported");
    GD_CHECK_ARG(user_emb && item_emb && out_idx, "score_topk: null pointer");
    GD_CHECK_ARG((mask_indptr == nullptr) == (mask_indices == nullptr), "score_topk: mask indptr/indices mismatch");
    const StPlan p = st_plan(n_rows, n_items, k);
    const size_t need = p.nslab > 1 ? (size_t)n_rows * p.nslab * k * sizeof(u64) : 0;
    if (need > 0 && (ws == nullptr || ws_bytes < need)) {
        gdmcf_set_error("score_topk: workspace of %zu B, %zu needed (gdmcf_score_topk_ws_bytes)", ws_bytes, need);
        return GDMCF_E_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int vec = (d % 4 == 0) && (ldu % 4 == 0) && (ldi % 4 == 0) && gd_aligned16(user_emb) && gd_aligned16(item_emb);
    const size_t lds = (size_t)p.R * p.CAP * 8 + (size_t)p.R * (8 + 4) + (size_t)p.R * ST_BM_WORDS * 4;
    int NP = 2;
    while (NP < p.nslab * k) NP <<= 1;
    const size_t lds_merge = (size_t)NP * 8;
    const bool areg = d <= 64;
    static bool attr_set = false;
    if (!attr_set) {
        // (the selection kernel also has 256 B of static LDS: the reduction behind __syncthreads_or)
        const void* fns[6] = {reinterpret_cast<const void*>(&score_topk_kernel<4, true>), reinterpret_cast<const void*>(&score_topk_kernel<4, false>),
                              reinterpret_cast<const void*>(&score_topk_kernel<2, true>), reinterpret_cast<const void*>(&score_topk_kernel<2, false>),
                              reinterpret_cast<const void*>(&score_topk_kernel<1, true>), reinterpret_cast<const void*>(&score_topk_kernel<1, false>)};
        bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&score_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      160 * 1024) == hipSuccess;
        for (int i = 0; i < 6; ++i) ok = ok && hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024) == hipSuccess;
        if (!ok) {
            gdmcf_set_error("score_topk: hipFuncSetAttribute failed");
            return GDMCF_E_HIP;
        }
        attr_set = true;
    }
    const int tiles = gd_cdiv(n_rows, p.R);
    const dim3 grid((unsigned)tiles * (unsigned)p.nslab);
    u64* wsp = reinterpret_cast<u64*>(ws);
    {
        GdProfScope prof(12, 2.0 * n_rows * (double)n_items * d, s);  // (both launches)
#define GD_ST_LAUNCH(RB_, AR_) hipLaunchKernelGGL((score_topk_kernel<RB_, AR_>), grid, dim3(256), lds, s, user_emb, ldu, user_ids, n_rows, item_emb, \
                                                   ldi, n_items, d, mask_indptr, mask_indices, k, p.R, p.CAP, p.nslab, p.slab_items, vec, out_idx, \
                                                   out_val, wsp)
        if (p.RB == 4 && areg) GD_ST_LAUNCH(4, true);
        else if (p.RB == 4) GD_ST_LAUNCH(4, false);
        else if (p.RB == 2 && areg) GD_ST_LAUNCH(2, true);
        else if (p.RB == 2) GD_ST_LAUNCH(2, false);
        else if (areg) GD_ST_LAUNCH(1, true);
        else GD_ST_LAUNCH(1, false);
#undef GD_ST_LAUNCH
        if (p.nslab > 1)
            hipLaunchKernelGGL(score_merge_kernel, dim3(n_rows), dim3(256), lds_merge, s, wsp, p.nslab * k, NP, k, out_idx, out_val);
    }
    return gd_launch_status("score_topk");
}

}  // extern "C"
