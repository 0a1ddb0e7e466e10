// Ranking metrics in float64 (reference evaluate_utils.py:6-52): the per-user terms from ranked lists and from ranks.
#include "common.h"

namespace {

// ---- ranking metrics (reference evaluate_utils.py:6-52) -----------------------------------------------------------
// One thread per user walks its K predicted items once, in rank order, exactly as the reference's inner loop does
// for every N (hits, dcg += 1/log2(j+2), ideal dcg over min(|GT|, N) ranks, reciprocal rank of the first hit), and
// emits the four per-user terms whenever j+1 reaches one of the requested cut-offs.  float64 throughout, additions
// in the reference's order: the per-user terms are bit-identical to the Python loop; the host adds them up in user
// order.  Ground-truth rows must have sorted column indices (binary search).
constexpr int TOPN_MAX = 8;
struct TopNList {
    int n;
    int v[TOPN_MAX];
};

__global__ __launch_bounds__(256) void topn_metrics_kernel(const int64_t* __restrict__ pred, int64_t ldp, int U,
                                                           const int64_t* __restrict__ gt_indptr,
                                                           const int32_t* __restrict__ gt_idx, const TopNList tn,
                                                           double* __restrict__ out) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= U) return;
    const int64_t beg = gt_indptr[u], end = gt_indptr[u + 1];
    const int64_t len = end - beg;
    double* o = out + (int64_t)u * tn.n * 4;
    if (len == 0) {
        for (int k = 0; k < tn.n * 4; ++k) o[k] = 0.0;
        return;
    }
    int hits = 0, next = 0;
    int64_t left = len;
    double dcg = 0.0, idcg = 0.0, mrr = 0.0;
    bool first = true;
    const int K = tn.v[tn.n - 1];
    for (int j = 0; j < K; ++j) {
        const int64_t item = pred[(int64_t)u * ldp + j];
        int64_t lo = beg, hi = end;  // lower bound of `item` in the sorted row
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)gt_idx[mid] < item) lo = mid + 1;
            else hi = mid;
        }
        const double gain = 1.0 / log2((double)(j + 2));
        if (lo < end && (int64_t)gt_idx[lo] == item) {
            dcg += gain;
            if (first) {
                mrr = 1.0 / ((double)j + 1.0);
                first = false;
            }
            ++hits;
        }
        if (left > 0) {
            idcg += gain;
            --left;
        }
        if (j + 1 == tn.v[next]) {
            const double N = (double)tn.v[next];
            o[next * 4 + 0] = (double)hits / N;
            o[next * 4 + 1] = (double)hits / (double)len;
            o[next * 4 + 2] = idcg != 0.0 ? dcg / idcg : 0.0;
            o[next * 4 + 3] = mrr;
            ++next;
        }
    }
}

// The same four terms from the RANKS of a user's ground-truth items (gdmcf_rank_targets_f32) instead of a list: one wave per user.
// The hits below a cut-off are visited in ascending rank -- every round the 64 lanes find the smallest (rank, column) pair not
// yet visited -- so dcg receives the gains topn_metrics_kernel adds, in its order; idcg runs over j < min(N, |GT|) in ascending
// j as there; the same expressions in float64: the same bits.  Every lane carries the same sums, lane 0 stores them.  Nothing
// is bounded by a list length: a cut-off past the last hit only closes the sums.
__global__ __launch_bounds__(256) void rank_metrics_kernel(const int32_t* __restrict__ ranks, int64_t ldr, int U, int G,
                                                           const TopNList tn, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= U) return;  // (the whole wave)
    const int32_t* r = ranks + (int64_t)u * ldr;
    int len = 0;
    for (int j = lane; j < G; j += 64) len += r[j] >= 0 ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) len += __shfl_xor(len, o);
    double* o = out + (int64_t)u * tn.n * 4;
    if (len == 0) {
        for (int k = lane; k < tn.n * 4; k += 64) o[k] = 0.0;
        return;
    }
    constexpr unsigned long long NONE = ~0ull;
    int hits = 0, next = 0, ji = 0;
    double dcg = 0.0, idcg = 0.0, mrr = 0.0;
    unsigned long long from = 0ull;  // pairs below it are visited
    while (next < tn.n) {
        unsigned long long best = NONE;
        for (int j = lane; j < G; j += 64) {
            const int32_t v = r[j];
            if (v >= 0) {
                const unsigned long long p = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)j;
                if (p >= from && p < best) best = p;
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long t = __shfl_xor(best, s);
            best = t < best ? t : best;
        }
        const int64_t rk = (int64_t)(best >> 32);  // (NONE: past every cut-off)
        while (next < tn.n && (best == NONE || rk >= (int64_t)tn.v[next])) {  // the cut-offs that close before this hit
            const int N = tn.v[next];
            for (; ji < N && ji < len; ++ji) idcg += 1.0 / log2((double)(ji + 2));
            if (lane == 0) {
                o[next * 4 + 0] = (double)hits / (double)N;
                o[next * 4 + 1] = (double)hits / (double)len;
                o[next * 4 + 2] = idcg != 0.0 ? dcg / idcg : 0.0;
                o[next * 4 + 3] = mrr;
            }
            ++next;
        }
        if (best == NONE) break;
        dcg += 1.0 / log2((double)(rk + 2));
        if (hits == 0) mrr = 1.0 / ((double)rk + 1.0);
        ++hits;
        from = best + 1ull;
    }
}

}  // namespace

extern "C" {

int gdmcf_topn_metrics_f64(const int64_t* pred_idx, int64_t ldp, int U, const int64_t* gt_indptr, const int32_t* gt_indices,
                           const int* topN_host, int n_topn, double* out, void* stream) {
    GD_CHECK_SHAPE(U > 0 && n_topn >= 1 && n_topn <= TOPN_MAX, "topn_metrics: bad shape (1..8 cut-offs)");
    GD_CHECK_ARG(pred_idx && gt_indptr && gt_indices && topN_host && out, "topn_metrics: null pointer");
    TopNList tn;
    tn.n = n_topn;
    for (int i = 0; i < n_topn; ++i) {
        tn.v[i] = topN_host[i];
        GD_CHECK_ARG(tn.v[i] >= 1 && (i == 0 || tn.v[i] > tn.v[i - 1]), "topn_metrics: cut-offs must be ascending and >= 1");
    }
    GD_CHECK_SHAPE(ldp >= tn.v[n_topn - 1], "topn_metrics: fewer predicted items per user than the largest cut-off");
    hipLaunchKernelGGL(topn_metrics_kernel, dim3(gd_cdiv(U, 256)), dim3(256), 0, (hipStream_t)stream, pred_idx, ldp, U,
                       gt_indptr, gt_indices, tn, out);
    return gd_launch_status("topn_metrics");
}

int gdmcf_rank_metrics_f64(const int32_t* ranks, int64_t ldr, int U, int G, const int* topN_host, int n_topn, double* out,
                           void* stream) {
    GD_CHECK_SHAPE(U > 0 && G >= 1 && ldr >= G && n_topn >= 1 && n_topn <= TOPN_MAX,
                   "gdmcf_rank_metrics_f64: bad shape (U > 0, G >= 1, ldr >= G, 1..8 cut-offs)");
    GD_CHECK_ARG(ranks && topN_host && out, "gdmcf_rank_metrics_f64: null pointer");
    TopNList tn;
    tn.n = n_topn;
    for (int i = 0; i < n_topn; ++i) {
        tn.v[i] = topN_host[i];
        GD_CHECK_ARG(tn.v[i] >= 1 && (i == 0 || tn.v[i] > tn.v[i - 1]), "gdmcf_rank_metrics_f64: cut-offs must be ascending and >= 1");
    }
    hipLaunchKernelGGL(rank_metrics_kernel, dim3(gd_cdiv(U, 4)), dim3(256), 0, (hipStream_t)stream, ranks, ldr, U, G, tn, out);
    return gd_launch_status("gdmcf_rank_metrics_f64");
}

}  // extern "C"
