// Masked per-row top-k (reference main.py:296-301).  Bound by HBM / cache bandwidth.
#include <stdlib.h>

#include "common.h"
#include "rank_order.h"

namespace {

// ---------------------------------------------------------------------------------------------
// masked top-k: one 256-thread workgroup per row.
//   1. history mask -> bitmap in LDS (I bits)
//   2. 4-pass 8-bit radix select on order-preserving uint32 keys -> k-th largest key (rank_order.h: order_key, masked_key)
//   3. collect keys > threshold (any order) + the lowest-index ties == threshold
//   4. bitonic sort of (key, ~index) pairs -> descending score, ascending index on ties
// ---------------------------------------------------------------------------------------------
// gdmcf_topk_masked_rows_f32: what the row-indirected instantiations take behind the plain kernels' arguments.  Both kernels
// below end in a parameter pack EXT that is either empty -- gdmcf_topk_masked_f32: the parameter list, the kernel arguments and
// the code are what they were without the pack -- or one TopkRowsArgs.
struct TopkRowsArgs {
    const int64_t* indptr2;   // second CSR (or nullptr)
    const int32_t* indices2;
    const int64_t* rows;      // [B] row of both CSRs per pred row (nullptr: the pred row's own number)
    const float* scale;       // [B] factor of the returned values (nullptr: none)
};
__device__ __forceinline__ const TopkRowsArgs& rows_args(const TopkRowsArgs& e) { return e; }

// NT threads per row: 1024 when the row is staged in LDS (the staged row allows one workgroup per CU anyway, and
// the select is a chain of short LDS loops -- 16 waves hide their latency, 4 waves measured 2.4x slower)
template <bool STAGE, int NT, class... EXT>
__global__ __launch_bounds__(NT) void topk_kernel(const float* __restrict__ pred, int64_t ldp, int I,
                                                   const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices, int k, int KP,
                                                   int64_t* __restrict__ idx_out, float* __restrict__ val_out, int redo,
                                                   const EXT... ext) {
    constexpr bool ROWS = sizeof...(EXT) != 0;
    // redo: second launch behind topk_fast_kernel -- only the rows it marked (first index -1) are selected here
    if (redo && idx_out[(int64_t)blockIdx.x * k] != -1) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(smem_raw);  // [KP]
    uint32_t* hist = reinterpret_cast<uint32_t*>(cand + KP);                     // [256]
    uint32_t* ctl = hist + 256;                                                  // [24]: 4 scalars + one count per wave
    uint32_t* bitmap = ctl + 24;                                                 // [ceil(I/32)]
    const int tid = threadIdx.x;
    const int row_id = blockIdx.x;
    const float* row = pred + (int64_t)row_id * ldp;
    const int nwords = (I + 31) >> 5;
    uint32_t* keys = bitmap + nwords;                                            // [I] when STAGE
    // key of element i: from the LDS copy when the row fits (one global pass, 8 loads in flight per thread),
    // otherwise recomputed from global memory in every pass
    auto KEY = [&](int i) -> uint32_t { return STAGE ? keys[i] : masked_key(row, bitmap, i); };

    for (int w = tid; w < nwords; w += NT) bitmap[w] = 0u;
    for (int j = tid; j < KP; j += NT) cand[j] = 0ull;
    __syncthreads();
    if constexpr (ROWS) {
        const TopkRowsArgs& e = rows_args(ext...);
        const int64_t mr = e.rows ? e.rows[row_id] : (int64_t)row_id;
        if (indptr) mask_row_bits<NT>(bitmap, I, indptr, indices, mr, tid);
        if (e.indptr2) mask_row_bits<NT>(bitmap, I, e.indptr2, e.indices2, mr, tid);
    } else if (indptr) {
        const int64_t beg = indptr[row_id], end = indptr[row_id + 1];
        for (int64_t j = beg + tid; j < end; j += NT) {
            const int c = indices[j];
            if (c >= 0 && c < I) atomicOr(&bitmap[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
    if (STAGE) {
        int i = tid;
        for (; i + 7 * NT < I; i += 8 * NT) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = row[i + u * NT];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = i + u * NT;
                keys[e] = (bitmap[e >> 5] & (1u << (e & 31))) ? NEG_INF_KEY : order_key(v[u]);
            }
        }
        for (; i < I; i += NT) keys[i] = masked_key(row, bitmap, i);
        __syncthreads();
    }

    // radix select
    uint32_t prefix = 0, pmask = 0;
    int need = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        // Scores cluster (pass 1 sees ~2 exponent bins), so plain LDS atomics would serialise on one counter:
        // every thread counts the bin of a sampled key privately and only the other bins go through atomics.
        const uint32_t guess = (KEY(I >> 1) >> shift) & 255u;
        uint32_t local = 0;
        __syncthreads();
        for (int i = tid; i < I; i += NT) {
            const uint32_t key = KEY(i);
            if ((key & pmask) == prefix) {
                const uint32_t b = (key >> shift) & 255u;
                if (b == guess) ++local;
                else atomicAdd(&hist[b], 1u);
            }
        }
        if (local) atomicAdd(&hist[guess], local);
        __syncthreads();
        if (tid < 64) {
            // find the bin holding the need-th largest key: wave 0 scans the 256 bins from the top, 4 per lane,
            // with a shuffle prefix sum (a serial walk by one thread costs 256 dependent LDS reads per pass)
            const int lane = tid;
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = hist[255 - 4 * lane - j];
            const uint32_t sum4 = c[0] + c[1] + c[2] + c[3];
            uint32_t pre = sum4;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(pre, o);
                if (lane >= o) pre += t;
            }
            const unsigned long long hit = __ballot(pre >= (uint32_t)need);
            const int L = hit ? (__ffsll((long long)hit) - 1) : 63;
            if (lane == L) {
                uint32_t cum = pre - sum4;
                int j = 0;
                for (; j < 3; ++j) {
                    if (cum + c[j] >= (uint32_t)need) break;
                    cum += c[j];
                }
                ctl[0] = (uint32_t)(255 - 4 * lane - j);
                ctl[1] = cum;   // elements strictly above the bin (within the prefix)
                ctl[2] = c[j];  // elements in the bin
            }
        }
        __syncthreads();
        prefix |= ctl[0] << shift;
        pmask |= 255u << shift;
        need -= (int)ctl[1];
        __syncthreads();
    }
    const uint32_t thr = prefix;       // k-th largest key
    const int n_eq_total = (int)ctl[2];  // elements equal to thr
    const int n_gt = k - need;         // elements strictly greater
    // need = number of ties to take (>= 1)

    if (tid == 0) ctl[3] = 0u;
    __syncthreads();
    if (n_eq_total == need) {
        // no surplus ties: order of collection is irrelevant
        for (int i = tid; i < I; i += NT) {
            const uint32_t key = KEY(i);
            if (key >= thr) {
                const uint32_t slot = atomicAdd(&ctl[3], 1u);
                cand[slot] = ((unsigned long long)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
            }
        }
    } else {
        for (int i = tid; i < I; i += NT) {
            const uint32_t key = KEY(i);
            if (key > thr) {
                const uint32_t slot = atomicAdd(&ctl[3], 1u);
                cand[slot] = ((unsigned long long)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
            }
        }
        // ties in index order: chunked ordered scan, stop once `need` were taken
        int taken = 0;
        const int lane = tid & 63, wave = tid >> 6;
        for (int base = 0; base < I && taken < need; base += NT) {
            const int i = base + tid;
            const bool f = (i < I) && (KEY(i) == thr);
            const unsigned long long bal = __ballot(f);
            if (lane == 0) ctl[4 + wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            int before = 0;
            for (int w = 0; w < wave; ++w) before += (int)ctl[4 + w];
            int total = 0;
            for (int w = 0; w < NT / 64; ++w) total += (int)ctl[4 + w];
            const int rank = taken + before + (int)__popcll(bal & ((1ull << lane) - 1ull));
            if (f && rank < need)
                cand[n_gt + rank] = ((unsigned long long)thr << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
            taken += total;
            __syncthreads();
        }
    }
    __syncthreads();

    // bitonic sort, descending
    for (int size = 2; size <= KP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int j = tid; j < KP / 2; j += NT) {
                const int lo = ((j / stride) * stride * 2) + (j % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long a = cand[lo], b = cand[hi];
                if ((a < b) == desc) {
                    cand[lo] = b;
                    cand[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    if constexpr (ROWS) {  // the same list, the values times the row's factor
        const TopkRowsArgs& e = rows_args(ext...);
        const float sc = (val_out && e.scale) ? e.scale[row_id] : 1.f;
        for (int j = tid; j < k; j += NT) {
            const unsigned long long c = cand[j];
            idx_out[(int64_t)row_id * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull));
            if (val_out) {
                const float v = key_to_float((uint32_t)(c >> 32));
                val_out[(int64_t)row_id * k + j] = e.scale ? v * sc : v;
            }
        }
        return;
    }
    for (int j = tid; j < k; j += NT) {
        const unsigned long long c = cand[j];
        idx_out[(int64_t)row_id * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull));
        if (val_out) val_out[(int64_t)row_id * k + j] = key_to_float((uint32_t)(c >> 32));
    }
}

// ---------------------------------------------------------------------------------------------
// The fast path (round 4): no radix passes, no staged row.  A thread keeps the upper halves of its KPT keys of the row in REGISTERS and their
// maximum goes to LDS; the k-th largest of the NT thread maxima, L, is a lower bound of the k-th largest key of the row (k
// threads hold an element >= L), so every element of the answer -- and every tie of its last element -- is among the elements
// >= L: for score rows that is k plus a few.  They are collected with their indices and sorted as (key, ~index) pairs: descending
// score, ascending index among equal scores, the first k are the answer -- the same list as topk_kernel's, bit for bit.
// ~14 KB of LDS and < 64 registers: two 1024-thread workgroups per CU, 400 rows in one round; the 55 MB of scores are read once.
// When more than CAP elements are >= L (degenerate rows: all scores equal, the large ones all in a few threads' columns, k above
// the number of unmasked items) the row is marked -- first index -1 -- and topk_kernel selects it in the launch that follows.
// ---------------------------------------------------------------------------------------------
constexpr int TOPK_FAST_CAP = 1024;
template <int NT, int KPT, class... EXT>
__global__ __launch_bounds__(NT, 8) void topk_fast_kernel(const float* __restrict__ pred, int64_t ldp, int I,
                                                         const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                         int k, int64_t* __restrict__ idx_out, float* __restrict__ val_out,
                                                         const EXT... ext) {
    constexpr bool ROWS = sizeof...(EXT) != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long* cand = reinterpret_cast<unsigned long long*>(smem_raw);  // [TOPK_FAST_CAP]
    uint32_t* tmax = reinterpret_cast<uint32_t*>(cand + TOPK_FAST_CAP);         // [NT]
    uint32_t* ctl = tmax + NT;                                                   // [4]
    uint32_t* bitmap = ctl + 4;                                                  // [ceil(I/32)]
    const int tid = threadIdx.x;
    const int row_id = blockIdx.x;
    const float* row = pred + (int64_t)row_id * ldp;
    const int nwords = (I + 31) >> 5;
    for (int w = tid; w < nwords; w += NT) bitmap[w] = 0u;
    if (tid == 0) ctl[0] = 0u;
    __syncthreads();
    if constexpr (ROWS) {
        const TopkRowsArgs& e = rows_args(ext...);
        const int64_t mr = e.rows ? e.rows[row_id] : (int64_t)row_id;
        if (indptr) mask_row_bits<NT>(bitmap, I, indptr, indices, mr, tid);
        if (e.indptr2) mask_row_bits<NT>(bitmap, I, e.indptr2, e.indices2, mr, tid);
    } else if (indptr) {
        const int64_t beg = indptr[row_id], end = indptr[row_id + 1];
        for (int64_t j = beg + tid; j < end; j += NT) {
            const int c = indices[j];
            if (c >= 0 && c < I) atomicOr(&bitmap[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
    // the thread's elements tid + u NT: the UPPER HALVES of their keys stay in registers, two per register (the exact key of the
    // few elements whose upper half reaches the bound's is fetched again below: L2); eight loads in flight
    uint32_t kh[(KPT + 1) / 2];
#pragma unroll
    for (int u = 0; u < (KPT + 1) / 2; ++u) kh[u] = 0u;
    uint32_t best = 0u;
#pragma unroll
    for (int u0 = 0; u0 < KPT; u0 += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = tid + (u0 + j) * NT;
            v[j] = (u0 + j < KPT && i < I) ? row[i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (u0 + j < KPT) {
                const int i = tid + (u0 + j) * NT;
                // (key 0 -- below every real key -- past the end of the row)
                const uint32_t kk = (i < I) ? ((bitmap[i >> 5] & (1u << (i & 31))) ? NEG_INF_KEY : order_key(v[j])) : 0u;
                kh[(u0 + j) >> 1] |= (kk >> 16) << (16 * ((u0 + j) & 1));
                best = kk > best ? kk : best;
            }
        }
    }
    tmax[tid] = best;
    __syncthreads();
    // bitonic sort of the NT maxima, descending
    for (int size = 2; size <= NT; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < NT / 2) {
                const int lo = ((tid / stride) * stride * 2) + (tid % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const uint32_t a = tmax[lo], b = tmax[hi];
                if ((a < b) == desc) {
                    tmax[lo] = b;
                    tmax[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t L = tmax[k - 1];
    // collect every element >= L
    const uint32_t Lh = L >> 16;
#pragma unroll
    for (int u = 0; u < KPT; ++u) {
        const int i = tid + u * NT;
        const uint32_t h = (kh[u >> 1] >> (16 * (u & 1))) & 0xFFFFu;
        if (i < I && h >= Lh) {
            const uint32_t kk = masked_key(row, bitmap, i);  // the exact key
            if (kk >= L) {
                const uint32_t slot = atomicAdd(&ctl[0], 1u);
                if (slot < (uint32_t)TOPK_FAST_CAP) cand[slot] = ((unsigned long long)kk << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
            }
        }
    }
    __syncthreads();
    const uint32_t C = ctl[0];
    if (C > (uint32_t)TOPK_FAST_CAP) {  // too many: topk_kernel takes this row in the next launch
        if (tid == 0) idx_out[(int64_t)row_id * k] = -1;
        return;
    }
    // sort the candidates (padded with key 0 up to the next power of two >= C, at least k)
    int CP = 2;
    while (CP < (int)C || CP < k) CP <<= 1;
    for (int j = (int)C + tid; j < CP; j += NT) cand[j] = 0ull;
    __syncthreads();
    for (int size = 2; size <= CP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int j = tid; j < CP / 2; j += NT) {
                const int lo = ((j / stride) * stride * 2) + (j % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                const unsigned long long a = cand[lo], b = cand[hi];
                if ((a < b) == desc) {
                    cand[lo] = b;
                    cand[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    if constexpr (ROWS) {  // the same list, the values times the row's factor
        const TopkRowsArgs& e = rows_args(ext...);
        const float sc = (val_out && e.scale) ? e.scale[row_id] : 1.f;
        for (int j = tid; j < k; j += NT) {
            const unsigned long long c = cand[j];
            idx_out[(int64_t)row_id * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull));
            if (val_out) {
                const float v = key_to_float((uint32_t)(c >> 32));
                val_out[(int64_t)row_id * k + j] = e.scale ? v * sc : v;
            }
        }
        return;
    }
    for (int j = tid; j < k; j += NT) {
        const unsigned long long c = cand[j];
        idx_out[(int64_t)row_id * k + j] = (int64_t)(0xFFFFFFFFu - (uint32_t)(c & 0xFFFFFFFFull));
        if (val_out) val_out[(int64_t)row_id * k + j] = key_to_float((uint32_t)(c >> 32));
    }
}

// Both top-k entries: the fast path where it applies, then the radix-select kernel (alone, or for the rows the fast path marked).
// EXT is the kernels' own pack: empty (gdmcf_topk_masked_f32) or one TopkRowsArgs, handed on behind the plain arguments.
template <class... EXT>
int topk_launch(const char* what, const float* pred, int64_t ldp, int B, int I, const int64_t* mask_indptr,
                const int32_t* mask_indices, int k, int64_t* idx_out, float* val_out, hipStream_t stream, const EXT... ext) {
    int KP = 2;
    while (KP < k) KP <<= 1;
    const size_t lds_base = (size_t)KP * 8 + (256 + 24) * 4 + (size_t)((I + 31) / 32) * 4;
    GdProfScope prof(9, 4.0 * B * (double)I, stream);  // (both launches)
    // the fast path (topk_fast_kernel): rows up to 40 960 wide, k <= 256 -- followed by topk_kernel for the rows it marks
    static const int fast_on = gd_env_int("GDMCF_TOPK_FAST", 1);  // 0: the radix-select kernel only
    const bool fast = fast_on && k <= 256 && I <= 1024 * 40 && k <= I;
    if (fast) {
        const size_t lds_f = (size_t)TOPK_FAST_CAP * 8 + (1024 + 4) * 4 + (size_t)((I + 31) / 32) * 4;
        if (I <= 1024 * 8)
            hipLaunchKernelGGL((topk_fast_kernel<1024, 8, EXT...>), dim3(B), dim3(1024), lds_f, stream, pred, ldp, I, mask_indptr,
                               mask_indices, k, idx_out, val_out, ext...);
        else if (I <= 1024 * 34)
            hipLaunchKernelGGL((topk_fast_kernel<1024, 34, EXT...>), dim3(B), dim3(1024), lds_f, stream, pred, ldp, I, mask_indptr,
                               mask_indices, k, idx_out, val_out, ext...);
        else
            hipLaunchKernelGGL((topk_fast_kernel<1024, 40, EXT...>), dim3(B), dim3(1024), lds_f, stream, pred, ldp, I, mask_indptr,
                               mask_indices, k, idx_out, val_out, ext...);
    }
    const int redo = fast ? 1 : 0;
    // (behind the fast path the marked rows are rare: the variant that does not stage the row needs 6 KB of LDS instead of 140 and
    // its workgroups -- all but the marked ones return at once -- are dispatched many per CU)
    const bool stage = !redo && lds_base + (size_t)I * 4 <= 150 * 1024;
    const size_t lds = lds_base + (stage ? (size_t)I * 4 : 0);
    if (lds > 160 * 1024) {
        gdmcf_set_error("%s: row width %d needs %zu B of LDS (> 160 KiB)", what, I, lds);
        return GDMCF_E_UNSUPPORTED;
    }
    static bool attr_set = false;  // (one per instantiation of this function, for its own two kernels)
    if (!attr_set) {
        void (*const k_stage)(const float*, int64_t, int, const int64_t*, const int32_t*, int, int, int64_t*, float*, int, EXT...) =
            &topk_kernel<true, 1024, EXT...>;
        void (*const k_plain)(const float*, int64_t, int, const int64_t*, const int32_t*, int, int, int64_t*, float*, int, EXT...) =
            &topk_kernel<false, 1024, EXT...>;
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_stage), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            160 * 1024);
        hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(k_plain), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            160 * 1024);
        if (e1 != hipSuccess || e2 != hipSuccess) {
            gdmcf_set_error("%s: hipFuncSetAttribute failed", what);
            return GDMCF_E_HIP;
        }
        attr_set = true;
    }
    if (stage)
        hipLaunchKernelGGL((topk_kernel<true, 1024, EXT...>), dim3(B), dim3(1024), lds, stream, pred, ldp, I, mask_indptr,
                           mask_indices, k, KP, idx_out, val_out, redo, ext...);
    else
        hipLaunchKernelGGL((topk_kernel<false, 1024, EXT...>), dim3(B), dim3(1024), lds, stream, pred, ldp, I, mask_indptr,
                           mask_indices, k, KP, idx_out, val_out, redo, ext...);
    return gd_launch_status(what);
}

}  // namespace

extern "C" {

int gdmcf_topk_masked_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* mask_indptr,
                          const int32_t* mask_indices, int k, int64_t* idx_out, float* val_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldp >= I, "topk: bad shape");
    GD_CHECK_SHAPE(k >= 1 && k <= I, "topk: k out of range (selected index k out of range)");
    GD_CHECK_ARG(k <= 2048, "topk: k > 2048 unsupported");
    GD_CHECK_ARG((mask_indptr == nullptr) == (mask_indices == nullptr), "topk: mask indptr/indices mismatch");
    return topk_launch("topk", pred, ldp, B, I, mask_indptr, mask_indices, k, idx_out, val_out, (hipStream_t)stream);
}

int gdmcf_topk_masked_rows_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* indptr, const int32_t* indices,
                               const int64_t* indptr2, const int32_t* indices2, const int64_t* rows, const float* scale, int k,
                               int64_t* idx_out, float* val_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldp >= I, "gdmcf_topk_masked_rows_f32: bad shape (B > 0, I > 0, ldp >= I)");
    GD_CHECK_SHAPE(k >= 1 && k <= I, "gdmcf_topk_masked_rows_f32: k out of range (selected index k out of range)");
    GD_CHECK_ARG(k <= 2048, "gdmcf_topk_masked_rows_f32: k > 2048 unsupported");
    GD_CHECK_ARG((indptr == nullptr) == (indices == nullptr), "gdmcf_topk_masked_rows_f32: mask indptr/indices mismatch");
    GD_CHECK_ARG((indptr2 == nullptr) == (indices2 == nullptr), "gdmcf_topk_masked_rows_f32: second mask indptr/indices mismatch");
    GD_CHECK_ARG(indptr2 == nullptr || indptr != nullptr, "gdmcf_topk_masked_rows_f32: a second CSR needs the first");
    GD_CHECK_ARG(pred && idx_out, "gdmcf_topk_masked_rows_f32: null pred / idx_out");
    const TopkRowsArgs ext = {indptr2, indices2, rows, scale};
    return topk_launch("gdmcf_topk_masked_rows_f32", pred, ldp, B, I, indptr, indices, k, idx_out, val_out, (hipStream_t)stream,
                       ext);
}

}  // extern "C"
