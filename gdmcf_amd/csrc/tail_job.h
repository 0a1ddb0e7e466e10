// The step's three small launches between the loss product and the input gradient -- the row-partial reducer and the row scale of
// reduce.hip, the float64 loss tail of loss_tail.hip -- as device functions, each written for the block and the grid stride it runs
// under: their own kernels call them with their launch's, and dr_kn_kernel (gemm_dr_kn.hip) runs all three on ONE workgroup that
// its task list leaves idle (GdTailJob, gd_tail_job_run).  Same operations in the same order whoever calls: the same bits.
#pragma once

#include "common.h"
#include "gemm_launch.h"

namespace {

// rowsum[m] = sum_j rowpart[m, j]: one wave per row, lane-strided partials + xor tree (fixed order).  Block `blk` of `nblk` takes rows
// blk * 4 + wave, then every nblk * 4-th; U rows of a wave are in flight together (each with its own sum: the order per row is the same).
template <int U>
__device__ __forceinline__ void gd_rowpart_reduce_rows(const float* __restrict__ rowpart, int ld, int M, int nt,
                                                       float* __restrict__ rowsum, int blk, int nblk) {
    const int lane = threadIdx.x & 63, step = nblk * 4;
    for (int m0 = blk * 4 + (int)(threadIdx.x >> 6); m0 < M; m0 += step * U) {
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = 0.f;
        for (int j = lane; j < nt; j += 64) {
#pragma unroll
            for (int u = 0; u < U; ++u) s[u] += rowpart[(int64_t)min(m0 + u * step, M - 1) * ld + j];  // (rows past M: read, not stored)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            for (int o = 32; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o);
            if (lane == 0 && m0 + u * step < M) rowsum[m0 + u * step] = s[u];
        }
    }
}

// out[m, k] = A[m, k] * rs[m]; four columns per thread (16-byte accesses; rows need only 4-byte alignment on gfx950).  Block
// (bx, by) of (nbx, nby) takes the 1024 columns from bx * 1024 of row by, then every nbx-th / nby-th; U rows in flight together.
// column K of the scaled copy = the row scale itself: as one more column of the weight-gradient product's second operand it
// makes the bias gradient sum_m rs[m] dZ[m, n] column K of that product (gdmcf_linear_bwd_weight_f32)
template <int U>
__device__ __forceinline__ void gd_rowscale_rows(const float* __restrict__ A, int64_t lda, const float* __restrict__ rs, int M, int K,
                                                 float* __restrict__ out, int64_t ldo, unsigned short* __restrict__ out16,
                                                 int64_t ldo16, int bias_col, int bx, int nbx, int by, int nby) {
    for (int kb = bx; kb * 1024 < K; kb += nbx) {
        const int k = (kb * 256 + (int)threadIdx.x) * 4;
        for (int m0 = by; m0 < M; m0 += nby * U) {
            float r[U];
            f32x4 t[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = min(m0 + u * nby, M - 1);  // (rows past M: read, not stored)
                r[u] = rs[m];
                const float* a = A + (int64_t)m * lda + k;
                if (k + 3 < K) {
                    t[u] = *reinterpret_cast<const f32x4_u4*>(a);
                } else {
                    for (int j = 0; j < 4; ++j) t[u][j] = k + j < K ? a[j] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = m0 + u * nby;
                if (m >= M) break;
                if (bias_col && kb == 0 && threadIdx.x == 0) out[(int64_t)m * ldo + K] = r[u];
                if (k >= K) continue;
                float* o = out + (int64_t)m * ldo + k;
                const float v[4] = {t[u].x * r[u], t[u].y * r[u], t[u].z * r[u], t[u].w * r[u]};
                if (k + 3 < K) {
                    *reinterpret_cast<f32x4_u4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
                } else {
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) o[j] = v[j];
                }
                if (out16)
                    for (int j = 0; j < 4; ++j)
                        if (k + j < K) out16[(int64_t)m * ldo16 + k + j] = gd_bf16_bits(v[j]);
            }
        }
    }
}

// float64 loss tail + Lt-history FIFO (reference gaussian_diffusion.py:339-370)
// The reference appends row by row (FIFO of H per timestep, :355-368).  The end state only depends,
// per timestep t, on the order of the rows with ts == t: it is the last min(H, cnt+n_t) entries of
// [old entries..., new entries in batch order].  So every row computes its rank among the earlier
// rows with the same t (independent, pipelined LDS reads -- no serial dependency chain) and writes
// straight to its final slot.  Needs T*H doubles + B ints of LDS.  One workgroup, whatever its size.
__device__ __forceinline__ void lt_history_parallel(const int64_t* __restrict__ ts, const double* __restrict__ lu, int B, int T, int H,
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

// The loss tail on ONE workgroup of 256 threads; fin_lds: lt_lds_bytes(T, H, B) bytes of LDS, 16-byte aligned.
__device__ __forceinline__ void gd_row_loss_finish_block(const float* __restrict__ rowsum, const float* __restrict__ rowdiv,
                                                         const float* __restrict__ alpha, float* __restrict__ gradcoef,
                                                         const int64_t* __restrict__ ts, const double* __restrict__ weight_t,
                                                         const double* __restrict__ pt, int B, int T, int H, double* hist,
                                                         int64_t* cnt, int update, double* __restrict__ lu, double* __restrict__ loss,
                                                         double* __restrict__ loss_mean, float* __restrict__ rowscale_mean,
                                                         float inv_b, unsigned char* fin_lds) {
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

}  // namespace

// The three launches' arguments as one job (B rows each): what gd_rowpart_reduce, gdmcf_row_loss_finish_mean_f64 and
// gdmcf_rowscale_f32 take.  on == 0: no job.
struct GdTailJob {
    int on;
    int B;
    const float* rowpart;  // reducer: [B, ld_rowpart], nt partial sums per row -> rowsum
    int ld_rowpart, nt;
    float* rowsum;
    const float* rowdiv;  // loss tail
    const float* alpha;
    float* gradcoef;
    const int64_t* ts;
    const double* weight_t;
    const double* pt;
    int T, H, update;
    double* hist;
    int64_t* cnt;
    double* lu;
    double* loss;
    double* loss_mean;
    float* rowscale_mean;
    float inv_b;
    int K;  // row scale: out[:, :K] = rs . A[:, :K]
    const float* A;
    int64_t lda;
    const float* rs;
    float* out;
    int64_t ldo;
    unsigned short* out16;
    int64_t ldo16;
    int bias_col;
};

namespace {

// All of a job on the calling workgroup (256 threads, lds: lt_lds_bytes(T, H, B) bytes): the reducer over all rows, the loss tail
// on the rowsum it wrote, the row scale with what the tail wrote (rs may be its rowscale_mean).  Block barriers only: what one
// stage reads of the one before was written by this workgroup, whose waves share the CU's vector cache.
__device__ __forceinline__ void gd_tail_job_run(const GdTailJob& j, unsigned char* lds) {
    gd_rowpart_reduce_rows<8>(j.rowpart, j.ld_rowpart, j.B, j.nt, j.rowsum, 0, 1);
    __syncthreads();
    gd_row_loss_finish_block(j.rowsum, j.rowdiv, j.alpha, j.gradcoef, j.ts, j.weight_t, j.pt, j.B, j.T, j.H, j.hist, j.cnt, j.update,
                             j.lu, j.loss, j.loss_mean, j.rowscale_mean, j.inv_b, lds);
    __syncthreads();
    gd_rowscale_rows<8>(j.A, j.lda, j.rs, j.B, j.K, j.out, j.ldo, j.out16, j.ldo16, j.bias_col, 0, 1, 0, 1);
}

// dynamic LDS of the FIFO update (lt_history_parallel): T*H doubles, 2 T ints, B ints
inline size_t lt_lds_bytes(int T, int H, int B) { return (size_t)T * H * 8 + (size_t)T * 8 + (size_t)B * 4 + 16; }
constexpr size_t GD_LT_LDS_MAX = 150 * 1024;  // what the loss tail's entries accept (their kernels: gd_allow_big_lds, gemm_launch.h)

}  // namespace

// gemm_dr_kn.hip: gd_dr_kn_launch with `job` (on != 0) riding the launch's first wholly idle workgroup.  GD_DR_NOT_TAKEN, nothing
// launched and g as it was, when the kernel does not take the product OR the job cannot ride: GDMCF_KN_TAIL=0, no idle workgroup,
// more LDS than GD_LT_LDS_MAX.
int gd_dr_kn_launch_tail(GdGemm& g, const GdTailJob& job, hipStream_t s);
