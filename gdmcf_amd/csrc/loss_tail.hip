// The float64 tail of the loss: per-row loss, gradient coefficients and mean, the Lt-history FIFO update, and the importance
// sampler of the timesteps that reads that history -- each kernel with its C entry.
#include "draws.h"

namespace {

// float64 loss tail + Lt-history FIFO (reference gaussian_diffusion.py:339-370)
// The reference appends row by row (FIFO of H per timestep, :355-368).  The end state only depends,
// per timestep t, on the order of the rows with ts == t: it is the last min(H, cnt+n_t) entries of
// [old entries..., new entries in batch order].  So every row computes its rank among the earlier
// rows with the same t (independent, pipelined LDS reads -- no serial dependency chain) and writes
// straight to its final slot.  Needs T*H doubles + B ints of LDS.
__device__ void lt_history_parallel(const int64_t* __restrict__ ts, const double* __restrict__ lu, int B, int T, int H,
                                    double* hist, int64_t* cnt, unsigned char* lds_raw) {
    double* old = reinterpret_cast<double*>(lds_raw);           // [T*H]
    int* n_t = reinterpret_cast<int*>(old + (size_t)T * H);     // [T]
    int* c0 = n_t + T;                                          // [T]
    int* tsl = c0 + T;                                          // [B]
    const int tid = threadIdx.x, nth = blockDim.x;
    for (int i = tid; i < T * H; i += nth) old[i] = hist[i];
    for (int t = tid; t < T; t += nth) {
        n_t[t] = 0;
        c0[t] = (int)cnt[t];
    }
    for (int b = tid; b < B; b += nth) tsl[b] = (int)ts[b];
    __syncthreads();
    for (int b = tid; b < B; b += nth) atomicAdd(&n_t[tsl[b]], 1);
    __syncthreads();
    // old entries slide left by `drop`
    for (int i = tid; i < T * H; i += nth) {
        const int t = i / H, j = i % H;
        const int drop = max(0, c0[t] + n_t[t] - H);
        if (j < c0[t] && j - drop >= 0) hist[(int64_t)t * H + (j - drop)] = old[i];
    }
    // new entries
    for (int b = tid; b < B; b += nth) {
        const int t = tsl[b];
        int rank = 0;
        for (int p = 0; p < b; ++p) rank += (tsl[p] == t);
        const int drop = max(0, c0[t] + n_t[t] - H);
        const int pos = c0[t] + rank - drop;
        if (pos >= 0) hist[(int64_t)t * H + pos] = lu[b];
    }
    for (int t = tid; t < T; t += nth) cnt[t] = (int64_t)min(H, c0[t] + n_t[t]);
}

__global__ __launch_bounds__(256) void row_loss_finish_kernel(const float* __restrict__ rowsum,
                                                              const float* __restrict__ rowdiv,
                                                              const float* __restrict__ alpha,
                                                              float* __restrict__ gradcoef,
                                                              const int64_t* __restrict__ ts,
                                                              const double* __restrict__ weight_t,
                                                              const double* __restrict__ pt, int B, int T, int H,
                                                              double* hist, int64_t* cnt, int update,
                                                              double* __restrict__ lu, double* __restrict__ loss,
                                                              double* __restrict__ loss_mean, float* __restrict__ rowscale_mean,
                                                              float inv_b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fin_lds[];
    double part = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const float mse = rowsum[b] / rowdiv[b];  // f32 mean, as mean_flat on f32 (:335)
        const double l = weight_t[ts[b]] * (double)mse;  // f64 weight * f32 mse -> f64 (:352)
        lu[b] = l;
        const double lb = l / pt[b];  // (:370)
        loss[b] = lb;
        part += lb;
        if (gradcoef) {
            const float gc = (float)(2.0 * (alpha ? (double)alpha[b] : 1.0) * weight_t[ts[b]] / (pt[b] * (double)rowdiv[b]));
            gradcoef[b] = gc;
            // the mean reduction of main.py:348 has the constant upstream gradient 1/B: the row scale of its backward
            if (rowscale_mean) rowscale_mean[b] = gc * inv_b;
        }
    }
    if (loss_mean) {  // losses["loss"].mean() (main.py:348) in float64, fixed order: lane-strided sums, xor tree, waves 0..3
        double* s_part = reinterpret_cast<double*>(fin_lds);  // the FIFO update below re-initialises what it uses
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = part;
        __syncthreads();
        if (threadIdx.x == 0) *loss_mean = (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / (double)B;
    }
    __syncthreads();
    if (update) lt_history_parallel(ts, lu, B, T, H, hist, cnt, fin_lds);
}

__global__ __launch_bounds__(256) void lt_history_update_kernel(const int64_t* ts, const double* lu, int B, int T,
                                                                int H, double* hist, int64_t* cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fin_lds[];
    lt_history_parallel(ts, lu, B, T, H, hist, cnt, fin_lds);
}

// importance-sampled timesteps (reference gaussian_diffusion.py:373-397) in ONE launch, no host sync:
// uniform until every Lt_count == H, then p_t ~ sqrt(mean(Lt_history^2)) mixed with uniform_prob,
// inverse-CDF sampling with a Philox stream; pt = p[t]*T (float64), or 1 in the uniform phase.
__global__ __launch_bounds__(256) void sample_timesteps_kernel(const double* __restrict__ hist,
                                                               const int64_t* __restrict__ cnt, int T, int H, int B,
                                                               double uniform_prob, uint64_t seed, uint64_t offset,
                                                               int64_t* __restrict__ ts, double* __restrict__ pt,
                                                               double* __restrict__ p_out, const GdStepState* step_state) {
    if (step_state) offset = step_state->ts_offset;
    extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
    double* p = reinterpret_cast<double*>(st_lds);  // [T] probabilities, then inclusive CDF in cdf[]
    double* cdf = p + T;
    __shared__ int full;
    __shared__ double total;
    const int tid = threadIdx.x;
    if (tid == 0) full = 1;
    __syncthreads();
    for (int t = tid; t < T; t += 256)
        if (cnt[t] != H) full = 0;
    __syncthreads();
    const bool imp = (full != 0);
    if (imp) {
        for (int t = tid; t < T; t += 256) {
            double s = 0.0;
            for (int j = 0; j < H; ++j) {
                const double v = hist[(int64_t)t * H + j];
                s += v * v;
            }
            p[t] = sqrt(s / (double)H);
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int t = 0; t < T; ++t) s += p[t];
            total = s;
        }
        __syncthreads();
        for (int t = tid; t < T; t += 256) {
            double v = p[t] / total;
            v *= 1.0 - uniform_prob;
            v += uniform_prob / (double)T;
            p[t] = v;
            if (p_out) p_out[t] = v;
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int t = 0; t < T; ++t) {
                s += p[t];
                cdf[t] = s;
            }
        }
        __syncthreads();
    }
    for (int b = tid; b < B; b += 256) {
        const uint4 r = gd_philox_block((uint32_t)b, 0, GD_STREAM_TIMESTEPS, offset, gd_philox_key(seed));
        const double u = ((double)r.x * 4294967296.0 + (double)r.y) * (1.0 / 18446744073709551616.0);  // [0,1)
        int t;
        if (imp) {
            const double x = u * cdf[T - 1];
            int lo = 0, hi = T - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (cdf[mid] > x) hi = mid; else lo = mid + 1;
            }
            t = lo;
            pt[b] = p[t] * (double)T;
        } else {
            t = min((int)(u * (double)T), T - 1);
            pt[b] = 1.0;
        }
        ts[b] = t;
    }
}

// dynamic LDS of the FIFO update (lt_history_parallel): T*H doubles, 2 T ints, B ints
size_t lt_lds_bytes(int T, int H, int B) { return (size_t)T * H * 8 + (size_t)T * 8 + (size_t)B * 4 + 16; }

// raises `kernel`'s dynamic-LDS limit when `lds` needs more than the default 48 KiB, once per kernel (*done: the caller's static
// flag).  T = 1000 diffusion steps x 10 history entries need 88 KB.
template <class K>
bool gd_allow_big_lds(K* kernel, size_t lds, bool* done, const char* who) {
    if (*done || lds <= 48 * 1024) return true;
    *done = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    if (!*done) gdmcf_set_error("%s: hipFuncSetAttribute failed", who);
    return *done;
}

}  // namespace

extern "C" {

int gdmcf_row_loss_finish_f64(const float* rowsum, const float* rowdiv, const float* alpha, const int64_t* ts,
                              const double* weight_t, const double* pt, int B, int T, int H, double* Lt_history,
                              int64_t* Lt_count, int update_history, double* loss_unscaled, double* loss,
                              float* gradcoef, void* stream) {
    return gdmcf_row_loss_finish_mean_f64(rowsum, rowdiv, alpha, ts, weight_t, pt, B, T, H, Lt_history, Lt_count, update_history,
                                          loss_unscaled, loss, gradcoef, nullptr, nullptr, stream);
}

int gdmcf_row_loss_finish_mean_f64(const float* rowsum, const float* rowdiv, const float* alpha, const int64_t* ts,
                                   const double* weight_t, const double* pt, int B, int T, int H, double* Lt_history,
                                   int64_t* Lt_count, int update_history, double* loss_unscaled, double* loss,
                                   float* gradcoef, double* loss_mean, float* rowscale_mean, void* stream) {
    GD_CHECK_SHAPE(B > 0 && T > 0 && H > 0, "row_loss_finish: bad shape");
    GD_CHECK_ARG(rowsum && rowdiv && ts && weight_t && pt && loss_unscaled && loss, "row_loss_finish: null pointer");
    GD_CHECK_ARG(!update_history || (Lt_history && Lt_count), "row_loss_finish: update_history without the history");
    GD_CHECK_ARG(!rowscale_mean || gradcoef, "row_loss_finish: rowscale_mean needs gradcoef");
    const size_t lds = lt_lds_bytes(T, H, B);
    GD_CHECK_ARG(lds <= 150 * 1024, "row_loss_finish: T*H and B too large for the LDS-resident FIFO update (150 KiB)");
    static bool attr_set = false;
    if (!gd_allow_big_lds(row_loss_finish_kernel, lds, &attr_set, "row_loss_finish")) return GDMCF_E_HIP;
    hipLaunchKernelGGL(row_loss_finish_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, rowsum, rowdiv, alpha,
                       gradcoef, ts, weight_t, pt, B, T, H, Lt_history, Lt_count, update_history, loss_unscaled, loss,
                       loss_mean, rowscale_mean, 1.0f / (float)B);
    return gd_launch_status("row_loss_finish");
}

int gdmcf_lt_history_update(const int64_t* ts, const double* loss_unscaled, int B, int T, int H, double* Lt_history,
                            int64_t* Lt_count, void* stream) {
    GD_CHECK_SHAPE(B > 0 && T > 0 && H > 0, "lt_history_update: bad shape");
    GD_CHECK_ARG(ts && loss_unscaled && Lt_history && Lt_count, "lt_history_update: null pointer");
    const size_t lds = lt_lds_bytes(T, H, B);
    GD_CHECK_ARG(lds <= 150 * 1024, "lt_history_update: T*H and B too large for the LDS-resident FIFO update (150 KiB)");
    static bool attr_set = false;
    if (!gd_allow_big_lds(lt_history_update_kernel, lds, &attr_set, "lt_history_update")) return GDMCF_E_HIP;
    hipLaunchKernelGGL(lt_history_update_kernel, dim3(1), dim3(256), lds, (hipStream_t)stream, ts, loss_unscaled, B, T,
                       H, Lt_history, Lt_count);
    return gd_launch_status("lt_history_update");
}

int gdmcf_sample_timesteps(const double* Lt_history, const int64_t* Lt_count, int T, int H, int B,
                           double uniform_prob, uint64_t seed, uint64_t offset, int64_t* ts, double* pt, double* p_out,
                           void* stream) {
    GD_CHECK_SHAPE(B > 0 && T > 0 && H > 0, "sample_timesteps: bad shape");
    GD_CHECK_OFFSET(offset, "sample_timesteps");
    GD_CHECK_ARG(T <= 4096, "sample_timesteps: T > 4096 unsupported");
    hipLaunchKernelGGL(sample_timesteps_kernel, dim3(1), dim3(256), (size_t)T * 16, (hipStream_t)stream, Lt_history,
                       Lt_count, T, H, B, uniform_prob, seed, offset, ts, pt, p_out, t_gd_step_state);
    return gd_launch_status("sample_timesteps");
}

}  // extern "C"
