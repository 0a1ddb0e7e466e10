// What linear.hip calls around the dense products: the split-K slab reducer, the bias-gradient column sum, the row-partial
// reducer of the fused loss, the row scale (with its C entry) and the f32 -> bf16 shadow cast.  Fixed orders: deterministic.
#include "tail_job.h"

namespace {

// split-K slab reducers (fixed slab order -> deterministic)
// mode 0: out = act(sum + bias[n]);  mode 1: out = rowscale[m] * sum * (act ? 1 - aact^2 : 1)
// Four consecutive columns per thread (one 16-byte load per slab; the slab rows are 16-byte aligned, see
// gdmcf_linear_ws_bytes) -- the additions per element are in the same slab order as before.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slabs, int64_t slab_stride,
                                                            int splits, int64_t ld_slab, int M, int N, int mode,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ rowscale,
                                                            const float* __restrict__ aact, int64_t ldact, int act,
                                                            float* __restrict__ out, int64_t ldo,
                                                            unsigned short* __restrict__ out16, int64_t ldo16, int vec) {
    const int m = blockIdx.y;
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= N) return;
    float sv[4] = {0.f, 0.f, 0.f, 0.f};
    const float* p = slabs + (int64_t)m * ld_slab + n0;
    if (vec && n0 + 3 < N) {
        // eight slab loads in flight, added in slab order (a plain loop waits for every load before issuing the next:
        // 19 x the L2 latency was the whole 9 us of this kernel)
        for (int k0 = 0; k0 < splits; k0 += 8) {
            f32x4 t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                t[u] = (k0 + u < splits) ? *reinterpret_cast<const f32x4*>(p + (int64_t)(k0 + u) * slab_stride)
                                         : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (k0 + u < splits) { sv[0] += t[u].x; sv[1] += t[u].y; sv[2] += t[u].z; sv[3] += t[u].w; }
        }
    } else {
        for (int k = 0; k < splits; ++k)
            for (int j = 0; j < 4; ++j)
                if (n0 + j < N) sv[j] += p[(int64_t)k * slab_stride + j];
    }
    const float rs = (mode != 0 && rowscale) ? rowscale[m] : 1.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j;
        if (n >= N) break;
        float s = sv[j];
        if (mode == 0) {
            if (bias) s += bias[n];
            if (act == 1) s = tanhf(s);
        } else {
            if (rowscale) s *= rs;
            if (act == 1) {
                const float h = aact[(int64_t)m * ldact + n];
                s *= (1.f - h * h);
            }
        }
        out[(int64_t)m * ldo + n] = s;
        if (out16) out16[(int64_t)m * ldo16 + n] = gd_bf16_bits(s);
    }
}

// out[m, k] = A[m, k] * rs[m]: gd_rowscale_rows (tail_job.h), one workgroup per 1024 columns of a row
__global__ __launch_bounds__(256) void rowscale_kernel(const float* __restrict__ A, int64_t lda,
                                                       const float* __restrict__ rs, int M, int K,
                                                       float* __restrict__ out, int64_t ldo,
                                                       unsigned short* __restrict__ out16, int64_t ldo16, int bias_col) {
    gd_rowscale_rows<1>(A, lda, rs, M, K, out, ldo, out16, ldo16, bias_col, blockIdx.x, gridDim.x, blockIdx.y, gridDim.y);
}

// db[n] = sum_m rs[m]*dZ[m,n].  One workgroup per 64 columns; wave w sums rows w, w+4, ... (each row read
// is one coalesced 256-B segment, 8 of them in flight), then the four partial sums are added in wave order.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dZ, int64_t ld,
                                                     const float* __restrict__ rs, int M, int N,
                                                     float* __restrict__ db) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane;
    const int nc = min(n, N - 1);
    float s = 0.f;
    int m = wave;
    for (; m + 28 < M; m += 32) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = dZ[(int64_t)(m + 4 * j) * ld + nc] * (rs ? rs[m + 4 * j] : 1.f);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; m < M; m += 4) s += dZ[(int64_t)m * ld + nc] * (rs ? rs[m] : 1.f);
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && n < N) db[n] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}

// rowsum[m] = sum_j rowpart[m, j]: gd_rowpart_reduce_rows (tail_job.h), one wave per row
__global__ __launch_bounds__(256) void rowpart_reduce_kernel(const float* __restrict__ rowpart, int ld, int M, int nt,
                                                             float* __restrict__ rowsum) {
    gd_rowpart_reduce_rows<1>(rowpart, ld, M, nt, rowsum, blockIdx.x, gridDim.x);
}

typedef __bf16 gd_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned gd_pack_bf16(float lo, float hi) {
    gd_bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}
typedef unsigned int gd_u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float* __restrict__ src, int64_t ld, unsigned short* __restrict__ dst,
                                                        int64_t ld16, int64_t rows, int64_t cols) {
    const int64_t groups = (cols + 7) / 8;  // 8 columns = one 16-byte store
    const int64_t total = rows * groups;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = u / groups, c = (u - r * groups) * 8;
        const float* p = src + r * ld + c;
        float e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = (c + i < cols) ? p[i] : 0.f;
        gd_u32x4 w;
        w.x = gd_pack_bf16(e[0], e[1]);
        w.y = gd_pack_bf16(e[2], e[3]);
        w.z = gd_pack_bf16(e[4], e[5]);
        w.w = gd_pack_bf16(e[6], e[7]);
        *reinterpret_cast<gd_u32x4*>(dst + r * ld16 + c) = w;
    }
}
}  // namespace

extern "C" {

int gdmcf_rowscale_f32(const float* A, int64_t lda, const float* rowscale, int M, int K, float* out, int64_t ldo,
                       void* stream) {
    GD_CHECK_SHAPE(M > 0 && K > 0 && lda >= K && ldo >= K, "rowscale: bad shape");
    GdShadow sh;
    const bool has16 = gd_shadow_lookup(out, &sh) && sh.rows == M && sh.cols == K;
    const int bias_col = ldo > K;  // room for one more column: out[m, K] = rowscale[m] (see the kernel)
    hipLaunchKernelGGL(rowscale_kernel, dim3(gd_cdiv(K, 1024), M), dim3(256), 0, (hipStream_t)stream, A, lda,
                       rowscale, M, K, out, ldo, has16 ? (unsigned short*)sh.p16 : nullptr, has16 ? sh.ld16 : 0, bias_col);
    return gd_launch_status("rowscale");
}

}  // extern "C"

// ---- internal helpers used by linear.hip ---------------------------------------------------------
int gd_splitk_reduce(const float* slabs, int64_t slab_stride, int splits, int64_t ld_slab, int M, int N, int mode,
                     const float* bias, const float* rowscale, const float* aact, int64_t ldact, int act, float* out,
                     int64_t ldo, hipStream_t s) {
    GdShadow sh;
    const bool has16 = gd_shadow_lookup(out, &sh) && sh.rows == M && sh.cols == N;
    const int vec = (ld_slab % 4 == 0) && (slab_stride % 4 == 0) && gd_aligned16(slabs);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(gd_cdiv(N, 1024), M), dim3(256), 0, s, slabs, slab_stride,
                       splits, ld_slab, M, N, mode, bias, rowscale, aact, ldact, act, out, ldo,
                       has16 ? (unsigned short*)sh.p16 : nullptr, has16 ? sh.ld16 : 0, vec);
    return gd_launch_status("splitk_reduce");
}

int gd_colsum(const float* dZ, int64_t ld, const float* rs, int M, int N, float* db, hipStream_t s) {
    hipLaunchKernelGGL(colsum_kernel, dim3(gd_cdiv(N, 64)), dim3(256), 0, s, dZ, ld, rs, M, N, db);
    return gd_launch_status("colsum");
}

int gd_rowpart_reduce(const float* rowpart, int ld, int M, int nt, float* rowsum, hipStream_t s) {
    hipLaunchKernelGGL(rowpart_reduce_kernel, dim3(gd_cdiv(M, 4)), dim3(256), 0, s, rowpart, ld, M, nt, rowsum);
    return gd_launch_status("rowpart_reduce");
}

// ---- f32 -> bf16 shadow copy (gdmcf_bf16_shadow_sync; weights whose values changed outside the library) -------
int gd_cast_bf16(const float* src, int64_t ld, void* dst, int64_t ld16, int64_t rows, int64_t cols, hipStream_t s) {
    const int64_t total = rows * ((cols + 7) / 8);
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, src, ld,
                       (unsigned short*)dst, ld16, rows, cols);
    return gd_launch_status("cast_bf16");
}
