// The float64 tail of the loss: per-row loss, gradient coefficients and mean, the Lt-history FIFO update, and the importance
// sampler of the timesteps that reads that history -- each kernel with its C entry.
#include "draws.h"
#include "tail_job.h"

namespace {

// float64 loss tail + Lt-history FIFO: gd_row_loss_finish_block / lt_history_parallel (tail_job.h) on one workgroup
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
    gd_row_loss_finish_block(rowsum, rowdiv, alpha, gradcoef, ts, weight_t, pt, B, T, H, hist, cnt, update, lu, loss, loss_mean,
                             rowscale_mean, inv_b, fin_lds);
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
    GD_CHECK_ARG(lds <= GD_LT_LDS_MAX, "row_loss_finish: T*H and B too large for the LDS-resident FIFO update (150 KiB)");
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
    GD_CHECK_ARG(lds <= GD_LT_LDS_MAX, "lt_history_update: T*H and B too large for the LDS-resident FIFO update (150 KiB)");
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
