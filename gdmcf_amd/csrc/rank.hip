// gdmcf_rank_targets_f32: the exact position of named items (the held-out targets of an evaluation) in the masked, tie-broken
// order the top-k entries rank by (rank_order.h) -- the one quantity untruncated MRR, mean rank, AUC, Recall@N for any N and
// leave-one-out HR / NDCG are functions of.  One pass over the scores, as the top-k's; its cost does not grow with a k.
#include "common.h"
#include "rank_order.h"

namespace {

// One 1024-thread workgroup per row:
//   1. the mask rows -> bitmap in LDS (I bits); its population count gives n_live
//   2. per pass of up to GP targets: their (key, ~index) pairs, bitonic-sorted descending in LDS (out-of-range targets and the
//      padding up to a power of two carry pair 0, below every real pair, and sink to the end)
//   3. the row is streamed once with 16-byte loads; every element's pair is located among the sorted targets by binary search and
//      the counter of its gap is bumped: counter g = elements with exactly g targets at or above them.  Elements below the lowest
//      target -- most of a row when the targets rank high -- are counted in a register and skip search and atomic
//   4. an inclusive prefix sum over the counters: entry m = elements strictly above target m = its rank
//   5. every target column finds its own pair in the sorted list (lower bound: equal targets meet at one entry) and stores the rank
// Integer LDS atomics only: the sums do not depend on the order the waves arrive in, so the result is the same in every run.
constexpr int RK_NT = 1024;
constexpr int RK_GP_MAX = 1024;  // targets per pass (<= RK_NT: one thread per counter in the prefix sum)
constexpr int RK_CTL = 20;       // words: [0] masked items, [1..16] wave totals of the prefix sum

struct RankArgs {
    const float* pred;
    int64_t ldp;
    int I;
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* indptr2;
    const int32_t* indices2;
    const int64_t* tgt_indptr;
    const int32_t* tgt_indices;
    const int64_t* rows;
    int G, GP;
    int32_t* rank_out;
    int64_t ldr;
    int32_t* n_live_out;
};

__device__ __forceinline__ unsigned long long rank_pair(uint32_t key, int i) {
    return ((unsigned long long)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
}

__global__ __launch_bounds__(RK_NT) void rank_targets_kernel(const RankArgs g) {
    constexpr int NT = RK_NT;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned long long* sorted = reinterpret_cast<unsigned long long*>(smem_raw);  // [GP]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(sorted + g.GP);                   // [GP + 1]
    uint32_t* ctl = cnt + g.GP + 1;                                                // [RK_CTL]
    uint32_t* bitmap = ctl + RK_CTL;                                               // [ceil(I/32)]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, I = g.I;
    const float* row = g.pred + (int64_t)b * g.ldp;
    const int nwords = (I + 31) >> 5;
    const int64_t cr = g.rows ? g.rows[b] : (int64_t)b;  // the row of every CSR

    for (int w = tid; w < nwords; w += NT) bitmap[w] = 0u;
    if (tid == 0) ctl[0] = 0u;
    __syncthreads();
    if (g.indptr) mask_row_bits<NT>(bitmap, I, g.indptr, g.indices, cr, tid);
    if (g.indptr2) mask_row_bits<NT>(bitmap, I, g.indptr2, g.indices2, cr, tid);
    __syncthreads();
    if (g.n_live_out) {
        uint32_t pc = 0;
        for (int w = tid; w < nwords; w += NT) pc += (uint32_t)__popc(bitmap[w]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o);
        if (lane == 0 && pc) atomicAdd(&ctl[0], pc);
        __syncthreads();
        if (tid == 0) g.n_live_out[b] = I - (int)ctl[0];
    }

    const int64_t tbeg = g.tgt_indptr[cr];
    const int64_t tlen = g.tgt_indptr[cr + 1] - tbeg;
    const int len = (int)(tlen < (int64_t)g.G ? (tlen > 0 ? tlen : 0) : (int64_t)g.G);
    int32_t* out = g.rank_out + (int64_t)b * g.ldr;
    for (int j = len + tid; j < g.G; j += NT) out[j] = -1;

    // the pair of target t (in range), as the stream forms it for element t
    auto target_pair = [&](int t) -> unsigned long long { return rank_pair(masked_key(row, bitmap, t), t); };

    for (int base = 0; base < len; base += g.GP) {
        const int n = min(g.GP, len - base);
        int NP = 2;
        while (NP < n) NP <<= 1;
        const int32_t* tg = g.tgt_indices + tbeg + base;
        for (int j = tid; j < NP; j += NT) {
            unsigned long long p = 0ull;
            if (j < n) {
                const int t = tg[j];
                if (t >= 0 && t < I) p = target_pair(t);
            }
            sorted[j] = p;
        }
        for (int j = tid; j <= NP; j += NT) cnt[j] = 0u;
        __syncthreads();
        for (int size = 2; size <= NP; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int j = tid; j < NP / 2; j += NT) {
                    const int lo = ((j / stride) * stride * 2) + (j % stride);
                    const int hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const unsigned long long a = sorted[lo], c = sorted[hi];
                    if ((a < c) == desc) {
                        sorted[lo] = c;
                        sorted[hi] = a;
                    }
                }
                __syncthreads();
            }
        }
        int nv = 0;  // targets in range: the entries ahead of the first pair 0
        {
            int lo = 0, hi = NP;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sorted[mid] != 0ull) lo = mid + 1;
                else hi = mid;
            }
            nv = lo;
        }
        if (nv > 0) {
            const unsigned long long lowest = sorted[nv - 1];
            uint32_t below = 0;
            auto count = [&](int i, float v, uint32_t masked) {
                const unsigned long long p = rank_pair(masked ? NEG_INF_KEY : order_key(v), i);
                if (p < lowest) {
                    ++below;
                    return;
                }
                int lo = 0, hi = nv;  // number of targets at or above p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sorted[mid] >= p) lo = mid + 1;
                    else hi = mid;
                }
                atomicAdd(&cnt[lo], 1u);
            };
            // four 16-byte loads in flight per thread (rows are only 4-byte aligned: odd strides)
            const int nq = I >> 2;
            int q = tid;
            for (; q + 3 * NT < nq; q += 4 * NT) {
                f32x4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f32x4_u4*>(row + 4 * (q + u * NT));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = 4 * (q + u * NT);
                    const uint32_t bits = bitmap[i >> 5] >> (i & 31);  // (four items of one word)
                    count(i, x[u].x, bits & 1u);
                    count(i + 1, x[u].y, bits & 2u);
                    count(i + 2, x[u].z, bits & 4u);
                    count(i + 3, x[u].w, bits & 8u);
                }
            }
            for (; q < nq; q += NT) {
                const f32x4 x = *reinterpret_cast<const f32x4_u4*>(row + 4 * q);
                const int i = 4 * q;
                const uint32_t bits = bitmap[i >> 5] >> (i & 31);
                count(i, x.x, bits & 1u);
                count(i + 1, x.y, bits & 2u);
                count(i + 2, x.z, bits & 4u);
                count(i + 3, x.w, bits & 8u);
            }
            for (int i = 4 * nq + tid; i < I; i += NT) count(i, row[i], (bitmap[i >> 5] >> (i & 31)) & 1u);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o);
            if (lane == 0 && below) atomicAdd(&cnt[nv], below);
        }
        __syncthreads();
        // inclusive prefix sum of cnt[0 .. NP): thread t owns counter t (NP <= GP <= NT)
        uint32_t v = tid < NP ? cnt[tid] : 0u;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(v, o);
            if (lane >= o) v += t;
        }
        if (lane == 63) ctl[1 + wave] = v;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += ctl[1 + w];
        if (tid < NP) cnt[tid] = v + before;
        __syncthreads();
        for (int j = tid; j < n; j += NT) {
            const int t = tg[j];
            int32_t r = -1;
            if (t >= 0 && t < I) {
                const unsigned long long p = target_pair(t);
                int lo = 0, hi = nv;  // number of targets strictly above p: the first entry that equals p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sorted[mid] > p) lo = mid + 1;
                    else hi = mid;
                }
                r = (int32_t)cnt[lo];
            }
            out[base + j] = r;
        }
        __syncthreads();  // (the next pass rewrites sorted / cnt)
    }
}

}  // namespace

extern "C" {

int gdmcf_rank_targets_f32(const float* pred, int64_t ldp, int B, int I, const int64_t* indptr, const int32_t* indices,
                           const int64_t* indptr2, const int32_t* indices2, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                           const int64_t* rows, int G, int32_t* rank_out, int64_t ldr, int32_t* n_live_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldp >= I, "gdmcf_rank_targets_f32: bad shape (B > 0, I > 0, ldp >= I)");
    GD_CHECK_SHAPE(G >= 1 && ldr >= G, "gdmcf_rank_targets_f32: bad shape (G >= 1, ldr >= G)");
    GD_CHECK_ARG((indptr == nullptr) == (indices == nullptr), "gdmcf_rank_targets_f32: mask indptr/indices mismatch");
    GD_CHECK_ARG((indptr2 == nullptr) == (indices2 == nullptr), "gdmcf_rank_targets_f32: second mask indptr/indices mismatch");
    GD_CHECK_ARG(indptr2 == nullptr || indptr != nullptr, "gdmcf_rank_targets_f32: a second CSR needs the first");
    GD_CHECK_ARG(pred && rank_out && tgt_indptr && tgt_indices, "gdmcf_rank_targets_f32: null pred / rank_out / targets");
    // targets per pass: what G needs, halved while the plan (sorted pairs, counters, bitmap) exceeds the LDS of a CU
    int GP = 2;
    while (GP < G && GP < RK_GP_MAX) GP <<= 1;
    const size_t lds_bitmap = (size_t)((I + 31) / 32) * 4;
    auto lds_of = [&](int gp) { return (size_t)gp * 8 + (size_t)(gp + 1 + RK_CTL) * 4 + lds_bitmap; };
    while (GP > 32 && lds_of(GP) > 160 * 1024) GP >>= 1;
    const size_t lds = lds_of(GP);
    if (lds > 160 * 1024) {
        gdmcf_set_error("gdmcf_rank_targets_f32: row width %d needs %zu B of LDS (> 160 KiB)", I, lds);
        return GDMCF_E_UNSUPPORTED;
    }
    static bool attr_set = false;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_targets_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024) != hipSuccess) {
            gdmcf_set_error("gdmcf_rank_targets_f32: hipFuncSetAttribute failed");
            return GDMCF_E_HIP;
        }
        attr_set = true;
    }
    const RankArgs g = {pred, ldp, I, indptr, indices, indptr2, indices2, tgt_indptr, tgt_indices, rows, G, GP, rank_out, ldr, n_live_out};
    hipLaunchKernelGGL(rank_targets_kernel, dim3(B), dim3(RK_NT), lds, (hipStream_t)stream, g);
    return gd_launch_status("gdmcf_rank_targets_f32");
}

}  // extern "C"
