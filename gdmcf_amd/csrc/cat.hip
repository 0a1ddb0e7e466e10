// The cat layer of the DNNCat backbone (reference models/DNN.py:180-265): `cat_layer = Linear(3, 1)` mixes, per user x item, the
// noised value x_t[b,i] with the two one-hot columns xU[b,2i], xU[b,2i+1] into one scalar in front of the plain DNN's layers.
//
//   gdmcf_cat_prep_input_f32   q_sample + mix + dropout in one pass over [B, I]: writes the item columns of the first layer's
//                              input and x_t (all the backward pass needs); the embedding columns, the padding and the 1 behind
//                              them are gdmcf_dnn_emb_cols_f32's (launched from the entry), so the layout of xin has one owner.
//   gdmcf_cat_grad_f32         the layer's four gradients from dxin = dZ1 . W1[:, 0:I]: one pass over [B, I] into per-workgroup
//                              float32 partials, then one workgroup that adds the partials in index order in float64.
//
// Evaluation order of the mix (float32, every operation rounded, no fused multiply-add -- nn.Linear's left-to-right dot product
// with the bias added last):
//       t = w0 * x_t;   t = t + w1 * xU0;   t = t + w2 * xU1;   z = t + c
// x_t and the dropout draws are the plain builder's (prep_input.hip) because both inline the same functions of draws.h:
// gd_normal4 + gd_qsample for x_t, gd_drop_block + gd_drop_bits (one block per PAIR of a thread's column groups) for the keep-mask.
//
// The drawn keep-mask is never stored: the backward pass recomputes it from (seed, offset) -- gdmcf_cat_grad_f32 takes the same
// drop_mode / keep / seed / offset as the builder.
//
// Mapping (both kernels): the plain builder's -- 256 threads, four columns per thread and group (one float4), CAT_G = PREP_G groups per
// thread 1024 columns apart, a workgroup per 4096 columns of a row; a thread's four items are eight consecutive floats of xU.
// No atomics: same inputs, same bits.
#include "draws.h"

namespace {

constexpr int CAT_G = PREP_G;
constexpr int CAT_SPAN = 256 * CAT_G * 4;  // columns of a row per workgroup

struct CatArgs {
    const float* x;  // x0 [B, ldx]
    int64_t ldx;
    const float* xU;  // one-hot image [B, ldu], item i in columns 2i, 2i + 1
    int64_t ldu;
    const int64_t* ts;
    const float* ca;
    const float* cb;
    int noise_mode;  // 0 none / 1 given / 2 Philox
    const float* noise;
    int64_t ldn;
    int drop_mode;  // 0 none / 1 given keep-mask / 2 Philox
    const uint8_t* keep;
    int64_t ldkeep;
    float drop_scale;      // 1/(1-p)
    uint32_t keep_thresh;  // keep iff (16-bit uniform) < keep_thresh
    uint64_t seed, offset;
    const float* cat_w;  // [3] device: parameters, read by the kernel
    const float* cat_b;  // [1]
    int B, I, one_col;   // one_col: column of xin that receives 1 (I + E), or -1
    float* xin;
    int64_t ldxin;
    float* xt;  // builder: out;  gradient: in
    int64_t ldxt;
    const float* dxin;  // gradient only
    int64_t lddx;
};

// the eight one-hot floats of items col .. col + 3
__device__ __forceinline__ void cat_load_u(const float* __restrict__ urow, int col, int I, bool full, float (&u)[8]) {
    if (full) {
        const f32x4 a = *reinterpret_cast<const f32x4_u4*>(urow + 2 * (int64_t)col);
        const f32x4 b = *reinterpret_cast<const f32x4_u4*>(urow + 2 * (int64_t)col + 4);
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w;
        u[4] = b.x; u[5] = b.y; u[6] = b.z; u[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = col + j < I;
            u[2 * j] = in ? urow[2 * (int64_t)(col + j)] : 0.f;
            u[2 * j + 1] = in ? urow[2 * (int64_t)(col + j) + 1] : 0.f;
        }
    }
}

// keep factors (0 or 1/(1-p)) of the four columns of group u; dr: the pair's Philox block (drop_mode 2)
__device__ __forceinline__ void cat_keep4(const CatArgs& a, int b, int col, int u, const uint4& dr, float (&k)[4]) {
    if (a.drop_mode == 1) {
        const uint8_t* kr = a.keep + (int64_t)b * a.ldkeep;
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (col + j < a.I && kr[col + j]) ? a.drop_scale : 0.f;
    } else if (a.drop_mode == 2) {
        uint32_t du[4];
        gd_drop_bits(dr, u & 1, du);
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (du[j] < a.keep_thresh) ? a.drop_scale : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = 1.f;
    }
}

__global__ __launch_bounds__(256) void cat_prep_kernel(CatArgs a) {
    const int b = blockIdx.y;
    float ca = 1.f, cb = 0.f;
    if (a.ca) {
        const int64_t t = a.ts[b];
        ca = a.ca[t];
        cb = a.cb[t];
    }
    const float w0 = a.cat_w[0], w1 = a.cat_w[1], w2 = a.cat_w[2], c = a.cat_b[0];
    const uint2 key = gd_philox_key(a.seed);
    const int col_base = (blockIdx.x * (256 * CAT_G) + threadIdx.x) * 4;
    const float* __restrict__ xr = a.x + (int64_t)b * a.ldx;
    const float* __restrict__ ur = a.xU + (int64_t)b * a.ldu;
    float* __restrict__ xin = a.xin + (int64_t)b * a.ldxin;
    float* __restrict__ xt = a.xt + (int64_t)b * a.ldxt;
    uint4 dr = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int u = 0; u < CAT_G; ++u) {
        const int col = col_base + u * 1024;
        if (a.drop_mode == 2 && (u & 1) == 0 && col < a.I) dr = gd_drop_block(col, b, a.offset, key);
        if (col >= a.I) continue;
        const bool full = col + 3 < a.I;
        float v[4], un[8], kp[4];
        gd_load4(xr, col, a.I, full, v);
        cat_load_u(ur, col, a.I, full, un);
        if (a.ca) {
            float nz[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.noise_mode == 1)
                gd_load4(a.noise + (int64_t)b * a.ldn, col, a.I, full, nz);
            else if (a.noise_mode == 2)
                gd_normal4(col, b, GD_STREAM_NOISE, a.offset, key, nz);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = gd_qsample(ca, v[j], cb, nz[j]);
        }
        cat_keep4(a, b, col, u, dr, kp);
        float z[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma clang fp contract(off)
            float t = w0 * v[j];
            const float t1 = w1 * un[2 * j];
            t = t + t1;
            const float t2 = w2 * un[2 * j + 1];
            t = t + t2;
            t = t + c;
            z[j] = (a.drop_mode == 0) ? t : (kp[j] != 0.f ? t * kp[j] : 0.f);
        }
        if (full) {
            *reinterpret_cast<f32x4*>(xt + col) = f32x4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f32x4*>(xin + col) = f32x4{z[0], z[1], z[2], z[3]};
        } else {
            for (int j = 0; j < 4; ++j)
                if (col + j < a.I) {
                    xt[col + j] = v[j];
                    xin[col + j] = z[j];
                }
        }
    }
    // the 1 behind the embedding columns (the bias column of the first layer's weight-gradient product), as the plain builder
    // leaves it; gdmcf_dnn_emb_cols_f32, which ran before this kernel on the same stream, wrote a zero there
    if (a.one_col >= 0 && blockIdx.x == 0 && threadIdx.x == 0) xin[a.one_col] = 1.f;
}

// gradients: first stage.  part[(b * gridDim.x + blockIdx.x) * 4 + k], k = (dz.x_t, dz.xU0, dz.xU1, dz)
__global__ __launch_bounds__(256) void cat_grad_kernel(CatArgs a, float* __restrict__ part) {
    const int b = blockIdx.y;
    const uint2 key = gd_philox_key(a.seed);
    const int col_base = (blockIdx.x * (256 * CAT_G) + threadIdx.x) * 4;
    const float* __restrict__ dr_ = a.dxin + (int64_t)b * a.lddx;
    const float* __restrict__ xt = a.xt + (int64_t)b * a.ldxt;
    const float* __restrict__ ur = a.xU + (int64_t)b * a.ldu;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    uint4 dr = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int u = 0; u < CAT_G; ++u) {
        const int col = col_base + u * 1024;
        if (a.drop_mode == 2 && (u & 1) == 0 && col < a.I) dr = gd_drop_block(col, b, a.offset, key);
        if (col >= a.I) continue;
        const bool full = col + 3 < a.I;
        float d[4], v[4], un[8], kp[4];
        gd_load4(dr_, col, a.I, full, d);
        gd_load4(xt, col, a.I, full, v);
        cat_load_u(ur, col, a.I, full, un);
        cat_keep4(a, b, col, u, dr, kp);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dz = (col + j < a.I) ? d[j] * kp[j] : 0.f;
            s0 += dz * v[j];
            s1 += dz * un[2 * j];
            s2 += dz * un[2 * j + 1];
            s3 += dz;
        }
    }
    // wave: xor shuffles (a fixed tree); workgroup: one LDS exchange, the four waves added in order
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
        s3 += __shfl_xor(s3, o);
    }
    __shared__ float red[4][4];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wv][0] = s0; red[wv][1] = s1; red[wv][2] = s2; red[wv][3] = s3;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        part[((int64_t)b * gridDim.x + blockIdx.x) * 4 + k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    }
}

// second stage: thread t adds partials t, t + 256, ... in this order in float64, then a fixed LDS tree; rounded once to float32
__global__ __launch_bounds__(256) void cat_grad_reduce_kernel(const float* __restrict__ part, int n, float* __restrict__ gw,
                                                               float* __restrict__ gb) {
    __shared__ double s[4][256];
    const int tid = threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += 256) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(part + 4 * (int64_t)j);
        acc[0] += (double)p.x; acc[1] += (double)p.y; acc[2] += (double)p.z; acc[3] += (double)p.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k][tid] = acc[k];
    __syncthreads();
    for (int m = 128; m > 0; m >>= 1) {
        if (tid < m) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k][tid] += s[k][tid + m];
        }
        __syncthreads();
    }
    if (tid < 3) gw[tid] = (float)s[tid][0];
    if (tid == 3) gb[0] = (float)s[3][0];
}

int cat_fill_drop(CatArgs& a, int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset) {
    a.drop_mode = drop_mode; a.keep = keep; a.ldkeep = ldkeep;
    gd_drop_params(drop_p, &a.drop_scale, &a.keep_thresh);
    a.seed = seed; a.offset = offset;
    return 0;
}

}  // namespace

extern "C" {

int gdmcf_cat_prep_input_f32(const float* x, int64_t ldx, const float* xU, int64_t ldu, const int64_t* ts, const float* ca,
                             const float* cb, int noise_mode, const float* noise, int64_t ldn, int drop_mode, const uint8_t* keep,
                             int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, const float* cat_w, const float* cat_b,
                             const float* emb_w, const float* emb_b, int E, int B, int I, float* xin, int64_t ldxin, float* xt_out,
                             int64_t ldxt, float* temb_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E > 0 && I <= 0x3FFFFFFF, "cat_prep_input: empty batch / no embedding columns / too many items");
    GD_CHECK_SHAPE(ldxin >= (int64_t)I + E && (ldxin % 4) == 0 && gd_aligned16(xin), "cat_prep_input: xin must be 16B aligned, ld%4==0, ld >= I+E");
    GD_CHECK_SHAPE(ldxt >= I && (ldxt % 4) == 0 && gd_aligned16(xt_out), "cat_prep_input: x_t must be 16B aligned, ld%4==0, ld >= I");
    GD_CHECK_SHAPE(ldx >= I && ldu >= 2 * (int64_t)I, "cat_prep_input: ldx < I or ldu < 2I");
    GD_CHECK_ARG(x && xU && xin && xt_out && cat_w && cat_b && ts && emb_w && emb_b, "cat_prep_input: null pointer");
    GD_CHECK_ARG((ca == nullptr) == (cb == nullptr), "cat_prep_input: ca/cb must both be set or both NULL");
    GD_CHECK_ARG(noise_mode >= 0 && noise_mode <= 2 && drop_mode >= 0 && drop_mode <= 2, "cat_prep_input: bad mode");
    GD_CHECK_ARG(!ca || noise_mode != 1 || (noise && ldn >= I), "cat_prep_input: explicit noise missing");
    GD_CHECK_ARG(drop_mode != 1 || (keep && ldkeep >= I), "cat_prep_input: explicit keep-mask missing");
    GD_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "cat_prep_input: dropout p out of range");
    // the Philox offset is a by-value argument: this entry has no device-side step state to read it from
    GD_CHECK_ARG(t_gd_step_state == nullptr, "cat_prep_input: not available while a graph step state is bound");
    // embedding columns, temb and the zero padding: the one kernel that owns that part of xin's layout
    int rc = gdmcf_dnn_emb_cols_f32(ts, emb_w, emb_b, E, B, I, xin, ldxin, temb_out, stream);
    if (rc) return rc;
    CatArgs a = {};
    a.x = x; a.ldx = ldx; a.xU = xU; a.ldu = ldu; a.ts = ts; a.ca = ca; a.cb = cb; a.noise_mode = ca ? noise_mode : 0;
    a.noise = noise; a.ldn = ldn;
    cat_fill_drop(a, drop_mode, keep, ldkeep, drop_p, seed, offset);
    a.cat_w = cat_w; a.cat_b = cat_b; a.B = B; a.I = I; a.one_col = (I + E < ldxin) ? I + E : -1;
    a.xin = xin; a.ldxin = ldxin; a.xt = xt_out; a.ldxt = ldxt;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(gd_cdiv(I, CAT_SPAN), B);
    {
        // algorithmic bytes: read x0 + the one-hot pair (+ explicit noise / keep-mask), write the item columns of xin and x_t
        const double bytes = (double)B * I * (4.0 + 8.0 + (a.noise_mode == 1 ? 4.0 : 0.0) + (drop_mode == 1 ? 1.0 : 0.0) + 8.0);
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL(cat_prep_kernel, grid, dim3(256), 0, s, a);
    }
    return gd_launch_status("cat_prep_input");
}

size_t gdmcf_cat_grad_ws_bytes(int B, int I) {
    if (B <= 0 || I <= 0) return 0;
    return (size_t)B * (size_t)gd_cdiv(I, CAT_SPAN) * 4 * sizeof(float);
}

int gdmcf_cat_grad_f32(const float* dxin, int64_t lddx, const float* xt, int64_t ldxt, const float* xU, int64_t ldu, int drop_mode,
                       const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, int B, int I, void* ws,
                       size_t ws_bytes, float* grad_w, float* grad_b, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && I <= 0x3FFFFFFF && lddx >= I && ldxt >= I && ldu >= 2 * (int64_t)I, "cat_grad: bad shape");
    GD_CHECK_ARG(dxin && xt && xU && grad_w && grad_b, "cat_grad: null pointer");
    GD_CHECK_ARG(drop_mode >= 0 && drop_mode <= 2 && (drop_mode != 1 || (keep && ldkeep >= I)), "cat_grad: bad mode / keep-mask missing");
    GD_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "cat_grad: dropout p out of range");
    GD_CHECK_ARG(t_gd_step_state == nullptr, "cat_grad: not available while a graph step state is bound");
    const int nbx = gd_cdiv(I, CAT_SPAN);
    GD_CHECK_SHAPE((int64_t)B * nbx < 2147483647LL / 4, "cat_grad: too many partials");
    if (ws == nullptr || ws_bytes < gdmcf_cat_grad_ws_bytes(B, I) || !gd_aligned16(ws)) {
        gdmcf_set_error("cat_grad: workspace %zu < %zu bytes (or not 16-byte aligned)", ws_bytes, gdmcf_cat_grad_ws_bytes(B, I));
        return GDMCF_E_WORKSPACE;
    }
    CatArgs a = {};
    a.xU = xU; a.ldu = ldu; a.xt = const_cast<float*>(xt); a.ldxt = ldxt; a.dxin = dxin; a.lddx = lddx; a.B = B; a.I = I;
    cat_fill_drop(a, drop_mode, keep, ldkeep, drop_p, seed, offset);
    hipStream_t s = (hipStream_t)stream;
    {
        // algorithmic bytes: read dxin, x_t and the one-hot pair (+ a given keep-mask)
        GdProfScope prof(7, (double)B * I * (4.0 + 4.0 + 8.0 + (drop_mode == 1 ? 1.0 : 0.0)), s);
        hipLaunchKernelGGL(cat_grad_kernel, dim3(nbx, B), dim3(256), 0, s, a, (float*)ws);
    }
    hipLaunchKernelGGL(cat_grad_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, B * nbx, grad_w, grad_b);
    return gd_launch_status("cat_grad");
}

}  // extern "C"
