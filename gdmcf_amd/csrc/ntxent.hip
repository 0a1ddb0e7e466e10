// The NT-Xent term between the two hidden activations of the embedding backbones (reference models/DNN.py:479-508, applied at
// :627-629) and its gradient with respect to both, without autograd, torch ops or a host round trip.  float32 throughout.
//
//   S = z1 z2^T / tau,  P = softmax of every row of S,  neg_i = sum_{j != i} P_ij,  term_i = -log((P_ii + eps) / neg_i),
//   closs = mean_i term_i
//   dS_ij = P_ij (g_ij - c_i) / tau  with  g_ii = -1 / (B (P_ii + eps)),  g_ij = 1 / (B neg_i),  c_i = sum_k g_ik P_ik
//   dz1 = scale dS z2,  dz2 = scale dS^T z1
//
// g_ij - c_i is formed without its cancellation (where P_ii << eps, 1 / neg_i and c_i B both round to 1 in float32): with
// w_i = (1 + eps) / (B tau (P_ii + eps)) and sum_j P_ij = 1,
//   (g_ii - c_i) / tau = -w_i,        (g_ij - c_i) / tau = w_i P_ii / neg_i   (j != i)
// -- the same numbers in exact arithmetic.  neg_i itself is the direct sum of the off-diagonal entries, never 1 - P_ii: when the
// diagonal dominates it is ~1e-9 and the subtraction would have no digits.
//
// Four launches, all latency bound ([B, B] and [B, d] data that lives in L2; B = 400, d = 1000 is 3 x 0.32 GFLOP):
//   (1) nx_scores_kernel    one wave per 16 x 16 tile of S on v_mfma_f32_16x16x4_f32, B^2 / 256 waves
//   (2) nx_softmax_kernel   one wave per row: maximum, exponentials, sum, P normalised in place, the row's three statistics
//   (3) nx_mean_kernel      closs = mean of the B terms in index order (one workgroup, as the other reducers here)
//   (4) nx_grad_kernel      both products, one wave per 16 rows x 64 columns of dz1 or dz2; dS is formed from P and the row
//                           statistics while the MFMA operand is loaded (dz2 reads P by columns)
// Every sum has one fixed order (k order of the products, xor trees over the lanes, strided partials of the mean) and nothing
// uses a float atomic: same inputs, same bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int NX_MAX = 4096;  // B and d

inline int nx_pad16(int n) { return (n + 15) & ~15; }

// workspace: P [B, ldp] (ldp = B rounded up to 16), then u, v, term [ldp] each:
//   u_i = (g_ij - c_i) / tau for j != i,  v_i = (g_ii - c_i) / tau,  term_i
struct NxWs {
    float* P;
    int ldp;
    float *u, *v, *term;
};

inline NxWs nx_ws(void* ws, int B) {
    NxWs w;
    w.ldp = nx_pad16(B);
    w.P = static_cast<float*>(ws);
    w.u = w.P + (size_t)B * w.ldp;
    w.v = w.u + w.ldp;
    w.term = w.v + w.ldp;
    return w;
}

// elements k .. k + 3 of a row of n floats; zeros behind n and for a row that does not exist (what follows the n elements in
// memory is not the row's and is never read)
__device__ __forceinline__ f32x4 nx_load4(const float* __restrict__ row, int k, int n, bool live) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (live) {
        if (k + 3 < n) {
            v = *reinterpret_cast<const f32x4_u4*>(row + k);
        } else {
            if (k < n) v.x = row[k];
            if (k + 1 < n) v.y = row[k + 1];
            if (k + 2 < n) v.z = row[k + 2];
        }
    }
    return v;
}

// ---------------------------------------------------------------------------------------------
// (1) S = z1 z2^T / tau.  Lane l of a wave holds row l & 15 of both 16-row operand blocks and, per step of 16 k, the four
// elements k0 + 4 (l >> 4) + s: MFMA s of the step multiplies the k with that s (the k order of the sum, the same for every tile).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nx_scores_kernel(const float* __restrict__ z1, int64_t ld1, const float* __restrict__ z2,
                                                         int64_t ld2, int B, int d, float tau, float* __restrict__ P, int ldp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = blockIdx.y * 16, c0 = (blockIdx.x * 4 + wave) * 16;
    if (c0 >= B) return;  // (no barrier in this kernel)
    const int lr = lane & 15, lq = lane >> 4;
    const bool live_a = r0 + lr < B, live_b = c0 + lr < B;
    const float* __restrict__ pa = z1 + (int64_t)min(r0 + lr, B - 1) * ld1;
    const float* __restrict__ pb = z2 + (int64_t)min(c0 + lr, B - 1) * ld2;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < d; k0 += 16) {
        const f32x4 a = nx_load4(pa, k0 + 4 * lq, d, live_a), b = nx_load4(pb, k0 + 4 * lq, d, live_b);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    // C layout: column = lane & 15, row = 4 (lane >> 4) + register.  Columns in [B, ldp) are the row's padding: zero.
    const int col = c0 + lr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = r0 + 4 * lq + r;
        if (row < B) P[(int64_t)row * ldp + col] = col < B ? acc[r] / tau : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// (2) one wave per row of S, in place: lane l owns columns l, l + 64, ... in all three passes (it re-reads only what it wrote)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float nx_wave_sum(float x) {
    for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

__global__ __launch_bounds__(256) void nx_softmax_kernel(float* __restrict__ P, int ldp, int B, float tau, float eps,
                                                          float* __restrict__ u, float* __restrict__ v, float* __restrict__ term) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;  // (whole waves leave; no barrier)
    float* __restrict__ row = P + (int64_t)i * ldp;
    float mx = -INFINITY;
    for (int j = lane; j < B; j += 64) mx = fmaxf(mx, row[j]);
    for (int m = 32; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    float sum = 0.f;
    for (int j = lane; j < B; j += 64) {
        const float e = expf(row[j] - mx);
        row[j] = e;
        sum += e;
    }
    sum = nx_wave_sum(sum);
    float neg = 0.f, pii = 0.f;
    for (int j = lane; j < B; j += 64) {
        const float p = row[j] / sum;
        row[j] = p;
        if (j == i) pii = p; else neg += p;
    }
    neg = nx_wave_sum(neg);
    pii = nx_wave_sum(pii);  // (one lane holds it, the others 0)
    if (lane == 0) {
        const float w = (1.f + eps) / ((float)B * tau * (pii + eps));
        term[i] = -logf((pii + eps) / neg);
        u[i] = w * pii / neg;
        v[i] = -w;
    }
}

// ---------------------------------------------------------------------------------------------
// (3) closs = mean_i term_i: thread t adds i = t, t + 256, ... in this order, then a fixed LDS tree
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nx_mean_kernel(const float* __restrict__ term, int B, float* __restrict__ out) {
    __shared__ float s[256];
    const int tid = threadIdx.x;
    float a = 0.f;
    for (int i = tid; i < B; i += 256) a += term[i];
    s[tid] = a;
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (tid < m) s[tid] += s[tid + m];
        __syncthreads();
    }
    if (tid == 0) *out = s[0] / (float)B;
}

// ---------------------------------------------------------------------------------------------
// (4) out[16 rows, 64 columns] = scale * A X with A = dS (dz1, X = z2) or dS^T (dz2, X = z1), K = B.  Lane l: row l & 15 of A,
// k = k0 + 4 (l >> 4) + s for MFMA s of a step of 16 k; of X the same four k, column l & 15 of each of the wave's four column tiles.
// ---------------------------------------------------------------------------------------------
template <bool TR>
__device__ __forceinline__ void nx_grad_tile(const float* __restrict__ P, int ldp, const float* __restrict__ u,
                                             const float* __restrict__ v, const float* __restrict__ X, int64_t ldx, int B, int d,
                                             float scale, float* __restrict__ out, int64_t ldo, int r0, int c0, int lane) {
    const int lr = lane & 15, lq = lane >> 4;
    const int arow = r0 + lr;  // i of dz1, j of dz2
    const bool live = arow < B;
    const int arow_c = min(arow, B - 1);
    float ui = 0.f, vi = 0.f;
    if (!TR) {
        ui = u[arow_c];
        vi = v[arow_c];
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < B; k0 += 16) {
        const int kb = k0 + 4 * lq;  // (kb + 3 < ldp: whole 16-byte pieces of P's rows and of u, v exist; only k < B is used)
        float a[4];
        if (!TR) {
            const f32x4 p = *reinterpret_cast<const f32x4*>(P + (int64_t)arow_c * ldp + kb);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = (live && kb + s < B) ? p[s] * (kb + s == arow ? vi : ui) : 0.f;
        } else {
            const f32x4 uk = *reinterpret_cast<const f32x4*>(u + kb), vk = *reinterpret_cast<const f32x4*>(v + kb);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int k = kb + s;
                a[s] = (live && k < B) ? P[(int64_t)k * ldp + arow] * (k == arow ? vk[s] : uk[s]) : 0.f;
            }
        }
        float x[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kb + s;
            const float* __restrict__ xr = X + (int64_t)min(k, B - 1) * ldx;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = c0 + 16 * t + lr;
                x[s][t] = (k < B && c < d) ? xr[c] : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], x[s][t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = c0 + 16 * t + lr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 4 * lq + r;
            if (row < B && c < d) out[(int64_t)row * ldo + c] = scale * acc[t][r];
        }
    }
}

__global__ __launch_bounds__(256) void nx_grad_kernel(const float* __restrict__ P, int ldp, const float* __restrict__ u,
                                                       const float* __restrict__ v, const float* __restrict__ z1, int64_t ld1,
                                                       const float* __restrict__ z2, int64_t ld2, int B, int d,
                                                       const float* __restrict__ scale_dev, float* __restrict__ dz1, int64_t lddz1,
                                                       float* __restrict__ dz2, int64_t lddz2) {
    const int lane = threadIdx.x & 63;
    const int r0 = blockIdx.y * 16, c0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (c0 >= d) return;  // (no barrier in this kernel)
    const float scale = scale_dev ? *scale_dev : 1.f;
    if (blockIdx.z == 0)
        nx_grad_tile<false>(P, ldp, u, v, z2, ld2, B, d, scale, dz1, lddz1, r0, c0, lane);
    else
        nx_grad_tile<true>(P, ldp, u, v, z1, ld1, B, d, scale, dz2, lddz2, r0, c0, lane);
}

int nx_check(const char* what, const void* z1, int64_t ld1, const void* z2, int64_t ld2, int B, int d, const void* ws,
             size_t ws_bytes) {
    if (B < 2 || B > NX_MAX || d < 1 || d > NX_MAX) {
        gdmcf_set_error("%s: 2 <= B <= %d and 1 <= d <= %d only (B = %d, d = %d)", what, NX_MAX, NX_MAX, B, d);
        return GDMCF_E_UNSUPPORTED;
    }
    GD_CHECK_SHAPE(ld1 >= d && ld2 >= d, "ntxent: leading dimension below d");
    GD_CHECK_ARG(z1 && z2 && ws, "ntxent: null pointer");
    GD_CHECK_ARG(gd_aligned16(ws), "ntxent: the workspace must be 16-byte aligned");
    if (ws_bytes < gdmcf_ntxent_ws_bytes(B)) {
        gdmcf_set_error("%s: workspace of %zu bytes, gdmcf_ntxent_ws_bytes(%d) = %zu", what, ws_bytes, B, gdmcf_ntxent_ws_bytes(B));
        return GDMCF_E_WORKSPACE;
    }
    return GDMCF_OK;
}

}  // namespace

extern "C" {

size_t gdmcf_ntxent_ws_bytes(int B) {
    if (B < 1) return 0;
    const size_t ldp = (size_t)nx_pad16(B);
    return ((size_t)B * ldp + 3 * ldp) * sizeof(float);
}

int gdmcf_ntxent_fwd_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int B, int d, float temperature, float eps,
                         void* ws, size_t ws_bytes, float* loss_out, void* stream) {
    const int rc = nx_check("ntxent_fwd", z1, ld1, z2, ld2, B, d, ws, ws_bytes);
    if (rc != GDMCF_OK) return rc;
    GD_CHECK_ARG(loss_out != nullptr, "ntxent_fwd: null pointer");
    GD_CHECK_ARG(temperature > 0.f && eps >= 0.f, "ntxent_fwd: temperature must be > 0 and eps >= 0");
    hipStream_t s = (hipStream_t)stream;
    const NxWs w = nx_ws(ws, B);
    const int nb = gd_cdiv(B, 16);
    hipLaunchKernelGGL(nx_scores_kernel, dim3(gd_cdiv(nb, 4), nb), dim3(256), 0, s, z1, ld1, z2, ld2, B, d, temperature, w.P, w.ldp);
    hipLaunchKernelGGL(nx_softmax_kernel, dim3(gd_cdiv(B, 4)), dim3(256), 0, s, w.P, w.ldp, B, temperature, eps, w.u, w.v, w.term);
    hipLaunchKernelGGL(nx_mean_kernel, dim3(1), dim3(256), 0, s, w.term, B, loss_out);
    return gd_launch_status("ntxent_fwd");
}

int gdmcf_ntxent_bwd_f32(const float* z1, int64_t ld1, const float* z2, int64_t ld2, int B, int d, const void* ws, size_t ws_bytes,
                         const float* scale, float* dz1, int64_t lddz1, float* dz2, int64_t lddz2, void* stream) {
    const int rc = nx_check("ntxent_bwd", z1, ld1, z2, ld2, B, d, ws, ws_bytes);
    if (rc != GDMCF_OK) return rc;
    GD_CHECK_ARG(dz1 && dz2, "ntxent_bwd: null pointer");
    GD_CHECK_SHAPE(lddz1 >= d && lddz2 >= d, "ntxent_bwd: leading dimension below d");
    const NxWs w = nx_ws(const_cast<void*>(ws), B);
    hipLaunchKernelGGL(nx_grad_kernel, dim3(gd_cdiv(d, 256), gd_cdiv(B, 16), 2), dim3(256), 0, (hipStream_t)stream, w.P, w.ldp, w.u,
                       w.v, z1, ld1, z2, ld2, B, d, scale, dz1, lddz1, dz2, lddz2);
    return gd_launch_status("ntxent_bwd");
}

}  // extern "C"
