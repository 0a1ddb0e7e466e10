// Row-wise HBM-bound kernels of the index backbones and the embedding gradients, each with its C entry: row norms, the backward
// of x / |x| (plain and fused with AdamW), tanh', row gather / scatter-add / scatter fused with AdamW, CSR row densify, scale, and
// the three kernels of the timestep-embedding gradient.
#include "common.h"

namespace {

// pieces of the indexIn backbone (reference models/DNN.py:510-682): embedding-row gather / scatter, row norms and
// the backward of x / |x| for the cosine scores, tanh' on a gradient with an extra addend.  All HBM-bound, one
// workgroup per row (16-byte accesses along the row), reductions in a fixed order (deterministic).
__device__ __forceinline__ float block_sum_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ X, int64_t ld, int cols,
                                                       float* __restrict__ norm, float* __restrict__ inv_norm) {
    __shared__ float red[4];
    const float* x = X + (int64_t)blockIdx.x * ld;
    float ss = 0.f;
    const int c4 = cols & ~3;
    for (int c = threadIdx.x * 4; c < c4; c += 1024) {
        const f32x4 t = *reinterpret_cast<const f32x4_u4*>(x + c);
        ss += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
    }
    if (threadIdx.x < cols - c4) ss += x[c4 + threadIdx.x] * x[c4 + threadIdx.x];
    const float n = sqrtf(block_sum_256(ss, red));
    if (threadIdx.x == 0) {
        if (norm) norm[blockIdx.x] = n;
        if (inv_norm) inv_norm[blockIdx.x] = 1.f / n;
    }
}

// dX = (dY - Y * <dY, Y>) * inv_norm  for Y = X / |X| (row-wise); dX may alias dY.  Rows of up to 4096 columns stay in
// registers between the dot product and the update (each operand is read once); longer rows are read twice.
// ADAM_: dX is not stored; it is the gradient of the AdamW update of X itself (row stride ldx, moments on the same stride),
// applied element by element in the same pass.  Both instances form dX with the same expressions in the same reduction
// order (the path is picked from `cols` alone), so the fused update sees exactly the gradient the plain instance stores.
template <bool ADAM_>
__global__ __launch_bounds__(256) void normalize_rows_bwd_kernel(const float* __restrict__ dY, int64_t lddy,
                                                                const float* __restrict__ Y, int64_t ldy,
                                                                const float* __restrict__ inv_norm, int cols,
                                                                float* __restrict__ dX, int64_t lddx,
                                                                float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                                GdAdamHyper h, const GdStepState* step_state) {
    __shared__ float red[4];
    if (ADAM_ && step_state) h = step_state->hyper;  // graph mode: this step's scalars from the device
    const float* dy = dY + (int64_t)blockIdx.x * lddy;
    const float* y = Y + (int64_t)blockIdx.x * ldy;
    float* dx = dX + (int64_t)blockIdx.x * lddx;
    float* mr = ADAM_ ? exp_avg + (int64_t)blockIdx.x * lddx : nullptr;
    float* vr = ADAM_ ? exp_avg_sq + (int64_t)blockIdx.x * lddx : nullptr;
    const float rn = inv_norm[blockIdx.x];
    if (cols <= 4096 && (cols & 3) == 0) {
        f32x4 a[4], b[4];
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = (threadIdx.x + 256 * k) * 4;
            a[k] = b[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c < cols) {
                a[k] = *reinterpret_cast<const f32x4_u4*>(dy + c);
                b[k] = *reinterpret_cast<const f32x4_u4*>(y + c);
            }
            dot += a[k].x * b[k].x + a[k].y * b[k].y + a[k].z * b[k].z + a[k].w * b[k].w;
        }
        dot = block_sum_256(dot, red);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = (threadIdx.x + 256 * k) * 4;
            if (c >= cols) continue;
            const f32x4 g = (a[k] - b[k] * dot) * rn;
            if (!ADAM_) {
                *reinterpret_cast<f32x4_u4*>(dx + c) = g;
                continue;
            }
            f32x4 pp = *reinterpret_cast<const f32x4_u4*>(dx + c);
            f32x4 mm = *reinterpret_cast<const f32x4_u4*>(mr + c);
            f32x4 vv = *reinterpret_cast<const f32x4_u4*>(vr + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pp[j], mj = mm[j], vj = vv[j];
                gd_adam_elem(pj, g[j], mj, vj, h);
                pp[j] = pj;
                mm[j] = mj;
                vv[j] = vj;
            }
            *reinterpret_cast<f32x4_u4*>(dx + c) = pp;
            *reinterpret_cast<f32x4_u4*>(mr + c) = mm;
            *reinterpret_cast<f32x4_u4*>(vr + c) = vv;
        }
        return;
    }
    float dot = 0.f;
    for (int c = threadIdx.x; c < cols; c += 256) dot += dy[c] * y[c];
    dot = block_sum_256(dot, red);
    for (int c = threadIdx.x; c < cols; c += 256) {
        const float g = (dy[c] - y[c] * dot) * rn;
        if (ADAM_)
            gd_adam_elem(dx[c], g, mr[c], vr[c], h);
        else
            dx[c] = g;
    }
}

__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ dA, int64_t ldd, const float* __restrict__ A,
                                                      int64_t lda, const float* __restrict__ extra, int64_t lde,
                                                      const float* __restrict__ scale, int N, float* __restrict__ out,
                                                      int64_t ldo) {
    const int m = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float g = dA[(int64_t)m * ldd + n];
    if (extra) g += scale[0] * extra[(int64_t)m * lde + n];
    const float a = A[(int64_t)m * lda + n];
    out[(int64_t)m * ldo + n] = g * (1.f - a * a);
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, int64_t lds,
                                                         const int64_t* __restrict__ index, int cols,
                                                         float* __restrict__ dst, int64_t ldd) {
    const float* s = src + index[blockIdx.x] * lds;
    float* d = dst + (int64_t)blockIdx.x * ldd;
    for (int c = threadIdx.x; c < cols; c += 256) d[c] = s[c];
}

__global__ __launch_bounds__(256) void scatter_add_rows_kernel(const float* __restrict__ src, int64_t lds,
                                                              const int64_t* __restrict__ index, int cols,
                                                              float* __restrict__ dst, int64_t ldd) {
    const float* s = src + (int64_t)blockIdx.x * lds;
    float* d = dst + index[blockIdx.x] * ldd;
    for (int c = threadIdx.x; c < cols; c += 256) atomicAdd(d + c, s[c]);  // (rows of one batch are distinct users)
}

// One pass over ALL rows of an embedding table W [rows, cols] (row stride ldw; exp_avg / exp_avg_sq on the same stride):
// AdamW with the dense gradient that scatter_add_rows would build in a zeroed table -- row index[j] takes 0 + src[j, :],
// every other row takes 0 (torch.optim.AdamW moves those rows too).  A workgroup owns SCATTER_ADAM_ROWS consecutive rows
// and finds the batch rows that land there by one scan of `index` (ids distinct within the batch, as above).
constexpr int SCATTER_ADAM_ROWS = 16;

__global__ __launch_bounds__(256) void scatter_rows_adamw_kernel(const float* __restrict__ src, int64_t lds,
                                                                const int64_t* __restrict__ index, int n, int rows, int cols,
                                                                float* __restrict__ W, int64_t ldw, float* __restrict__ exp_avg,
                                                                float* __restrict__ exp_avg_sq, GdAdamHyper h,
                                                                const GdStepState* step_state) {
    __shared__ int slot[SCATTER_ADAM_ROWS];
    if (step_state) h = step_state->hyper;  // graph mode: this step's scalars from the device
    const int64_t r0 = (int64_t)blockIdx.x * SCATTER_ADAM_ROWS;
    if (threadIdx.x < SCATTER_ADAM_ROWS) slot[threadIdx.x] = -1;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += 256) {
        const int64_t r = index[j] - r0;
        if (r >= 0 && r < SCATTER_ADAM_ROWS) slot[r] = j;
    }
    __syncthreads();
    const int nr = (int)min((int64_t)SCATTER_ADAM_ROWS, rows - r0);
    const bool vec = ((cols | ldw | lds) & 3) == 0 &&
                     ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(exp_avg) |
                       reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
    if (vec) {
        const int c4 = cols >> 2;
        for (int it = threadIdx.x; it < nr * c4; it += 256) {
            const int rr = it / c4, c = (it - rr * c4) * 4;
            const int j = slot[rr];
            const int64_t o = (r0 + rr) * ldw + c;
            f32x4 gg = {0.f, 0.f, 0.f, 0.f};
            if (j >= 0) gg = gg + *reinterpret_cast<const f32x4*>(src + (int64_t)j * lds + c);  // 0 + g: the zeroed table's sum
            f32x4 pp = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(W + o));
            f32x4 mm = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(exp_avg + o));
            f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(exp_avg_sq + o));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float pq = pp[q], mq = mm[q], vq = vv[q];
                gd_adam_elem(pq, gg[q], mq, vq, h);
                pp[q] = pq;
                mm[q] = mq;
                vv[q] = vq;
            }
            __builtin_nontemporal_store(pp, reinterpret_cast<f32x4*>(W + o));
            __builtin_nontemporal_store(mm, reinterpret_cast<f32x4*>(exp_avg + o));
            __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(exp_avg_sq + o));
        }
        return;
    }
    for (int it = threadIdx.x; it < nr * cols; it += 256) {
        const int rr = it / cols, c = it - rr * cols;
        const int j = slot[rr];
        const int64_t o = (r0 + rr) * ldw + c;
        float g = 0.f;
        if (j >= 0) g = g + src[(int64_t)j * lds + c];
        gd_adam_elem(W[o], g, exp_avg[o], exp_avg_sq[o], h);
    }
}

// W1e[n, e] = W1[n, I+e]: the E embedding columns of the first layer gathered into a compact [N, E] block
__global__ __launch_bounds__(256) void emb_gather_w_kernel(const float* __restrict__ W1, int64_t ldw, int I, int E, int N,
                                                           float* __restrict__ W1e) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < N * E) W1e[idx] = W1[(int64_t)(idx / E) * ldw + I + (idx % E)];
}

// demb[m,e] = sum_n dZ1[m,n] * W1e[n,e]   (one workgroup per row m, waves stride over e)
__global__ __launch_bounds__(256) void emb_bwd_demb_kernel(const float* __restrict__ dZ1, int64_t lddz,
                                                           const float* __restrict__ W1e, int E, int N,
                                                           float* __restrict__ demb) {
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = wave; e < E; e += 4) {
        float s = 0.f;
        for (int n = lane; n < N; n += 64) s += dZ1[(int64_t)m * lddz + n] * W1e[(int64_t)n * E + e];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) demb[(int64_t)m * E + e] = s;
    }
}

// dWe[e,f] = sum_m demb[m,e]*temb[m,f];  dbe[e] = sum_m demb[m,e]   (one wave per output element)
__global__ __launch_bounds__(64) void emb_bwd_w_kernel(const float* __restrict__ demb, const float* __restrict__ temb,
                                                       int M, int E, float* __restrict__ dWe,
                                                       float* __restrict__ dbe) {
    const int idx = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    if (idx < E * E) {
        const int e = idx / E, f = idx % E;
        for (int m = lane; m < M; m += 64) s += demb[(int64_t)m * E + e] * temb[(int64_t)m * E + f];
    } else {
        const int e = idx - E * E;
        for (int m = lane; m < M; m += 64) s += demb[(int64_t)m * E + e];
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) {
        if (idx < E * E) dWe[idx] = s;
        else dbe[idx - E * E] = s;
    }
}

// dense[b, :] = row row_ids[b] of a CSR matrix (values NULL -> 1.0).  One workgroup per row: 16-byte zero fill,
// barrier, scatter of the row's nonzeros.  Replaces scipy .todense() + a 55 MB host-to-device copy per batch.
__global__ __launch_bounds__(256) void densify_rows_kernel(const int64_t* __restrict__ indptr,
                                                           const int32_t* __restrict__ indices,
                                                           const float* __restrict__ values,
                                                           const int64_t* __restrict__ row_ids, int I,
                                                           float* __restrict__ out, int64_t ldo) {
    const int b = blockIdx.x;
    float* row = out + (int64_t)b * ldo;
    const bool al = ((reinterpret_cast<uintptr_t>(row) & 15u) == 0);
    if (al) {
        for (int i = threadIdx.x * 4; i + 3 < I; i += 1024) *reinterpret_cast<f32x4*>(row + i) = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int i = (I & ~3) + threadIdx.x; i < I; i += 256) row[i] = 0.f;
    } else {
        for (int i = threadIdx.x; i < I; i += 256) row[i] = 0.f;
    }
    __syncthreads();
    const int64_t u = row_ids ? row_ids[b] : b;
    for (int64_t j = indptr[u] + threadIdx.x; j < indptr[u + 1]; j += 256) {
        const int c = indices[j];
        if (c >= 0 && c < I) row[c] = values ? values[j] : 1.f;
    }
}

__global__ __launch_bounds__(256) void scale_kernel(const float* __restrict__ a, int64_t n, float s,
                                                    float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] * s;
}

}  // namespace

extern "C" {

int gdmcf_row_norms_f32(const float* X, int64_t ld, int rows, int cols, float* norm, float* inv_norm, void* stream) {
    GD_CHECK_SHAPE(rows > 0 && cols > 0 && ld >= cols, "row_norms: bad shape");
    GD_CHECK_ARG(X && (norm || inv_norm), "row_norms: null pointer");
    hipLaunchKernelGGL(row_norms_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, X, ld, cols, norm, inv_norm);
    return gd_launch_status("row_norms");
}

int gdmcf_normalize_rows_bwd_f32(const float* dY, int64_t lddy, const float* Y, int64_t ldy, const float* inv_norm, int rows,
                                 int cols, float* dX, int64_t lddx, void* stream) {
    GD_CHECK_SHAPE(rows > 0 && cols > 0 && lddy >= cols && ldy >= cols && lddx >= cols, "normalize_rows_bwd: bad shape");
    GD_CHECK_ARG(dY && Y && inv_norm && dX, "normalize_rows_bwd: null pointer");
    hipLaunchKernelGGL(normalize_rows_bwd_kernel<false>, dim3(rows), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy,
                       inv_norm, cols, dX, lddx, nullptr, nullptr, GdAdamHyper{}, nullptr);
    return gd_launch_status("normalize_rows_bwd");
}

int gdmcf_normalize_rows_bwd_adamw_f32(const float* dY, int64_t lddy, const float* Y, int64_t ldy, const float* inv_norm,
                                       int rows, int cols, float* X, int64_t ldx, float* exp_avg, float* exp_avg_sq, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                                       void* stream) {
    GD_CHECK_SHAPE(rows > 0 && cols > 0 && lddy >= cols && ldy >= cols && ldx >= cols, "normalize_rows_bwd_adamw: bad shape");
    GD_CHECK_ARG(dY && Y && inv_norm && X && exp_avg && exp_avg_sq && step >= 1, "normalize_rows_bwd_adamw: null pointer");
    const GdAdamHyper h = gd_adam_hyper(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    {
        // algorithmic bytes: read dY, Y, X, m, v; write X, m, v
        GdProfScope prof(6, 32.0 * (double)rows * cols, (hipStream_t)stream);
        hipLaunchKernelGGL(normalize_rows_bwd_kernel<true>, dim3(rows), dim3(256), 0, (hipStream_t)stream, dY, lddy, Y, ldy,
                           inv_norm, cols, X, ldx, exp_avg, exp_avg_sq, h, t_gd_step_state);
    }
    return gd_launch_status("normalize_rows_bwd_adamw");
}

int gdmcf_tanh_bwd_f32(const float* dA, int64_t ldd, const float* A, int64_t lda, const float* extra, int64_t lde,
                       const float* scale, int M, int N, float* out, int64_t ldo, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && ldd >= N && lda >= N && ldo >= N && (!extra || lde >= N), "tanh_bwd: bad shape");
    GD_CHECK_ARG(dA && A && out && (!extra || scale), "tanh_bwd: null pointer");
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(gd_cdiv(N, 256), M), dim3(256), 0, (hipStream_t)stream, dA, ldd, A, lda, extra, lde,
                       scale, N, out, ldo);
    return gd_launch_status("tanh_bwd");
}

int gdmcf_gather_rows_f32(const float* src, int64_t lds, const int64_t* index, int n, int cols, float* dst, int64_t ldd,
                          void* stream) {
    GD_CHECK_SHAPE(n > 0 && cols > 0 && lds >= cols && ldd >= cols, "gather_rows: bad shape");
    GD_CHECK_ARG(src && index && dst, "gather_rows: null pointer");
    hipLaunchKernelGGL(gather_rows_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, src, lds, index, cols, dst, ldd);
    return gd_launch_status("gather_rows");
}

int gdmcf_scatter_add_rows_f32(const float* src, int64_t lds, const int64_t* index, int n, int cols, float* dst, int64_t ldd,
                               void* stream) {
    GD_CHECK_SHAPE(n > 0 && cols > 0 && lds >= cols && ldd >= cols, "scatter_add_rows: bad shape");
    GD_CHECK_ARG(src && index && dst, "scatter_add_rows: null pointer");
    hipLaunchKernelGGL(scatter_add_rows_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, src, lds, index, cols, dst, ldd);
    return gd_launch_status("scatter_add_rows");
}

int gdmcf_scatter_rows_adamw_f32(const float* src, int64_t lds, const int64_t* index, int n, int rows, int cols, float* W,
                                 int64_t ldw, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, int step, float grad_scale, void* stream) {
    GD_CHECK_SHAPE(n >= 0 && rows > 0 && cols > 0 && ldw >= cols && (n == 0 || lds >= cols), "scatter_rows_adamw: bad shape");
    GD_CHECK_ARG(W && exp_avg && exp_avg_sq && (n == 0 || (src && index)) && step >= 1, "scatter_rows_adamw: null pointer");
    const GdAdamHyper h = gd_adam_hyper(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    {
        // algorithmic bytes: read W, m, v; write W, m, v (the batch rows' gradient is noise beside them)
        GdProfScope prof(6, 24.0 * (double)rows * cols, (hipStream_t)stream);
        hipLaunchKernelGGL(scatter_rows_adamw_kernel, dim3(gd_cdiv(rows, SCATTER_ADAM_ROWS)), dim3(256), 0, (hipStream_t)stream,
                           src, lds, index, n, rows, cols, W, ldw, exp_avg, exp_avg_sq, h, t_gd_step_state);
    }
    return gd_launch_status("scatter_rows_adamw");
}

int gdmcf_emb_bwd_f32(const float* dZ1, int64_t lddz, const float* W1, int64_t ldw, int I, int E, const float* temb,
                      int M, int N, float* demb_ws, float* dWe, float* dbe, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && E > 0 && I >= 0 && ldw >= I + E && lddz >= N, "emb_bwd: bad shape");
    GD_CHECK_ARG(dZ1 && W1 && temb && demb_ws && dWe && dbe, "emb_bwd: null pointer");
    hipStream_t s = (hipStream_t)stream;
    float* W1e = demb_ws + (size_t)M * E;  // demb_ws holds [M*E] demb followed by [N*E] gathered weights
    hipLaunchKernelGGL(emb_gather_w_kernel, dim3(gd_cdiv(N * E, 256)), dim3(256), 0, s, W1, ldw, I, E, N, W1e);
    hipLaunchKernelGGL(emb_bwd_demb_kernel, dim3(M), dim3(256), 0, s, dZ1, lddz, W1e, E, N, demb_ws);
    hipLaunchKernelGGL(emb_bwd_w_kernel, dim3(E * E + E), dim3(64), 0, s, demb_ws, temb, M, E, dWe, dbe);
    return gd_launch_status("emb_bwd");
}

int gdmcf_densify_rows_f32(const int64_t* indptr, const int32_t* indices, const float* values, const int64_t* row_ids,
                           int B, int I, float* out, int64_t ldo, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldo >= I, "densify_rows: bad shape");
    GD_CHECK_ARG(indptr && indices && out, "densify_rows: null pointer");
    hipLaunchKernelGGL(densify_rows_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, indptr, indices, values, row_ids,
                       I, out, ldo);
    return gd_launch_status("densify_rows");
}

int gdmcf_scale_f32(const float* acc, int64_t n, float scale, float* out, void* stream) {
    GD_CHECK_SHAPE(n > 0, "scale: empty");
    GD_CHECK_ARG(acc && out, "scale: null pointer");
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc, n,
                       scale, out);
    return gd_launch_status("scale");
}

}  // extern "C"
