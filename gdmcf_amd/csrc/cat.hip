// The cat layer of the DNNCat backbone (reference models/DNN.py:180-265): `cat_layer = Linear(3, 1)` mixes, per user x item, the
// noised value x_t[b,i] with the two one-hot columns xU[b,2i], xU[b,2i+1] into one scalar in front of the plain DNN's layers.
//
//   gdmcf_cat_prep_input_f32   q_sample + mix + dropout in one pass over [B, I]: writes the item columns of the first layer's
//                              input and x_t (all the backward pass needs); the embedding columns, the padding and the 1 behind
//                              them are gdmcf_dnn_emb_cols_f32's (launched from the entry), so the layout of xin has one owner.
//   gdmcf_cat_grad_f32         the layer's four gradients from dxin = dZ1 . W1[:, 0:I]: one pass over [B, I] into per-workgroup
//                              float32 partials, then one workgroup that adds the partials in index order in float64.
//   gdmcf_cat_prep_input_csr_f32   the builder fed from {0,1} CSR rows: the dense rows, the [B, 2I] one-hot image and the launch that
//                              draws its classes (onehot_noise_kernel) never exist.  The row is the workgroup's LDS bitmap of its
//                              4096 columns (as prep_input.hip marks it), the classes are drawn in place with onehot_noise_kernel's
//                              counter; rows and classes leave as two bitmaps, the loss target and the gradient's source.
//   gdmcf_cat_grad_bits_f32    gdmcf_cat_grad_f32 with the one-hot pair taken from those two bitmaps.
// Both are the SAME kernels as the dense ones, instantiated on another source (template <int SRC>): a compile-time choice, so
// that the dense instantiations' ISA is what it was and every value behind the source is formed by one piece of code.  The
// builder's outputs agree with the dense pair's bit for bit; the gradient's do too (see cat_grad_kernel for grad_w[0]).
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
// No global atomics: same inputs, same bits (the LDS bitmap is marked with atomicOr, which commutes).
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

// The source of a kernel is a compile-time choice (template <int SRC>): 0 = the dense operands of CatArgs, nothing more to pass.
struct CatDense {};

// CSR source of the builder (SRC 1): row b of the batch is row rows[b] of a {0,1} CSR matrix; CatArgs::x / xU are NULL then
struct CatCsr {
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* rows;
    const int64_t* ts_U;     // [B] timesteps of the class draws (may be NULL when the classes are given)
    const uint8_t* sampled;  // given classes [B, lds] or NULL: drawn (stream 3, offset_noise)
    int64_t lds;
    float p1_off;           // gd_p1_off(discrete)
    uint64_t offset_noise;  // Philox offset of the class draws (CatArgs::offset is the noise's and the dropout's)
    uint32_t* x0bits;       // out: the rows as bitmaps, word c >> 5, bit c & 31 = column c (0 behind I)
    int64_t ldx0bits;
    uint32_t* clsbits;  // out: the classes, same format
    int64_t ldclsbits;
};

// bitmap source of the gradient (SRC 1): what the CSR-fed builder left
struct CatBits {
    const uint32_t* x0bits;
    int64_t ldx0bits;
    const uint32_t* clsbits;
    int64_t ldclsbits;
};

// the eight one-hot floats of items col .. col + 3 from their classes as nibbles (bit j: item col + j): c0 the row's, s the
// drawn one -- the pair onehot_noise_kernel writes, (c0 == 0 && s == 0, c0 == 1 && s == 1); 0 behind I like cat_load_u
__device__ __forceinline__ void cat_pair_bits(uint32_t c0n, uint32_t sn, int col, int I, bool full, float (&u)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = full || col + j < I;
        const bool c0 = (c0n >> j) & 1u, s = (sn >> j) & 1u;
        u[2 * j] = (in && !c0 && !s) ? 1.f : 0.f;
        u[2 * j + 1] = (in && c0 && s) ? 1.f : 0.f;
    }
}

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

// SRC 0: dense rows and their one-hot image (S = CatDense).  SRC 1: CSR rows (S = CatCsr): x0 and the pair are formed from the
// workgroup's LDS bitmap and the class draw; everything behind them -- x_t, the mix, the dropout, the stores -- is this one body.
// The kernel itself is the template (not a body inlined into two wrappers, which gave the dense kernel another register
// allocation): the SRC 0 instantiation's ISA is instruction for instruction what the untemplated kernel's was (the gradient
// kernel's differs in one constant, the offset of its hidden launch arguments behind the empty source).
template <int SRC, class S>
__global__ __launch_bounds__(256) void cat_prep_kernel(CatArgs a, S s) {
    const int b = blockIdx.y;
    __shared__ uint32_t s_bm[SRC == 1 ? CAT_SPAN / 32 : 1];  // SRC 1: this workgroup's 4096 columns of row b as bits
    const int bm_col0 = blockIdx.x * CAT_SPAN;
    const int nwords = (a.I + 31) >> 5;
    if constexpr (SRC == 1) {
        // marked as prep_input_body does: zero the words, atomicOr the row's entries that fall in the span, barrier
        if (threadIdx.x < CAT_SPAN / 32) s_bm[threadIdx.x] = 0u;
        __syncthreads();
        const int64_t r = s.rows[b];
        const int64_t beg = s.indptr[r], end = s.indptr[r + 1];
        for (int64_t k = beg + threadIdx.x; k < end; k += 256) {
            const int ci = s.indices[k];
            const int c = ci - bm_col0;
            if (c >= 0 && c < CAT_SPAN && ci < a.I) atomicOr(&s_bm[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
        if (threadIdx.x < CAT_SPAN / 32) {
            const int w = (bm_col0 >> 5) + (int)threadIdx.x;
            if (w < nwords) s.x0bits[(int64_t)b * s.ldx0bits + w] = s_bm[threadIdx.x];
        }
    }
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
    // SRC 1: the classes of a group's four items (bit j: item col + j); a = ts_U[b] / B as onehot_noise_kernel scales it
    uint32_t cls[CAT_G] = {};
    float an = 1.f;
    if constexpr (SRC == 1) {
        if (!s.sampled) an = gd_class_scale(s.ts_U[b], a.B);
    }
#pragma unroll
    for (int u = 0; u < CAT_G; ++u) {
        const int col = col_base + u * 1024;
        if (a.drop_mode == 2 && (u & 1) == 0 && col < a.I) dr = gd_drop_block(col, b, a.offset, key);
        if (col >= a.I) continue;
        const bool full = col + 3 < a.I;
        float v[4], un[8], kp[4];
        if constexpr (SRC == 0) {
            gd_load4(xr, col, a.I, full, v);
            cat_load_u(ur, col, a.I, full, un);
        } else {
            // col is a multiple of 4: one word of the bitmap holds all four items (its bits behind I are 0)
            const uint32_t c0n = (s_bm[(col - bm_col0) >> 5] >> ((col - bm_col0) & 31)) & 15u;
            uint32_t sn = 0u;
            if (s.sampled) {
                const uint8_t* sr = s.sampled + (int64_t)b * s.lds;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((full || col + j < a.I) && sr[col + j]) sn |= 1u << j;
            } else {
                // onehot_noise_kernel's block for the four items col .. col + 3: a group needs exactly one
                const uint4 r = gd_philox_block((uint32_t)(col >> 2), b, GD_STREAM_ONEHOT_CLASS, s.offset_noise, key);
                const uint32_t cu[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (full || col + j < a.I) sn |= (uint32_t)gd_class_draw((c0n >> j) & 1u, an, s.p1_off, cu[j]) << j;
            }
            cls[u] = sn;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ((c0n >> j) & 1u) ? 1.f : 0.f;
            cat_pair_bits(c0n, sn, col, a.I, full, un);
        }
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
    if constexpr (SRC == 1) {
        // the classes as a bitmap: the eight lanes 8k .. 8k + 7 hold the 32 columns of one word of every group u (nibble
        // lane & 7).  All lanes are here again (the loop's `continue` left cls[u] = 0), so the nibbles are OR-ed by xor shuffles
        // and lane 8k stores the word.
#pragma unroll
        for (int u = 0; u < CAT_G; ++u) {
            uint32_t w = cls[u] << (4 * (threadIdx.x & 7));
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            const int wi = (bm_col0 >> 5) + u * 32 + (int)(threadIdx.x >> 3);
            if ((threadIdx.x & 7) == 0 && wi < nwords) s.clsbits[(int64_t)b * s.ldclsbits + wi] = w;
        }
    }
}

// gradients: first stage.  part[(b * gridDim.x + blockIdx.x) * 4 + k], k = (dz.x_t, dz.xU0, dz.xU1, dz)
// SRC 0: the pair from the one-hot image (S = CatDense).  SRC 1: from the two bitmaps (S = CatBits): a thread's four items are
// one nibble of word col >> 5 of each, one 4-byte load per bitmap and group.  The pair is exactly 0.f / 1.f either way and the
// sums run in the same order, so grad_w[1], grad_w[2] and grad_b equal the dense kernel's bit for bit whatever is fused (a
// product with 0.f or 1.f is exact).  grad_w[0] = sum dz * x_t depends on which products are fused into their sum.  The dense
// instantiation leaves that to the compiler (default contraction), and its results must stay what they are, so its source is
// not touched; what the compiler made of it is recorded in cat_grad_fused() below and SRC 1 writes that arithmetic out with
// contraction off.  A compiler that chooses differently for the dense kernel shows in
// tests/test_gpu_dnncat_csr.py::test_cat_grad_bits_equals_cat_grad_on_the_image_of_the_same_bits (I > 1024); the answer then
// is to read the dense kernel's ISA again (the v_pk_fma_f32 / v_pk_add_f32 chain of each group) and correct the table.
//
// dense instantiation, hipcc of ROCm 7.2 at -O3 for gfx950: s0 = fma(dz, x_t, s0) for every item, except items 1 and 2 of a
// thread's second group (u == 1), whose product is rounded before it is added (v_pk_mul_f32 + v_pk_add_f32)
__device__ __forceinline__ constexpr bool cat_grad_fused(int u, int j) { return !(u == 1 && (j == 1 || j == 2)); }

template <int SRC, class S>
__global__ __launch_bounds__(256) void cat_grad_kernel(CatArgs a, float* __restrict__ part, S s) {
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
        if constexpr (SRC == 0) {
            cat_load_u(ur, col, a.I, full, un);
        } else {
            const uint32_t c0n = (s.x0bits[(int64_t)b * s.ldx0bits + (col >> 5)] >> (col & 31)) & 15u;
            const uint32_t sn = (s.clsbits[(int64_t)b * s.ldclsbits + (col >> 5)] >> (col & 31)) & 15u;
            cat_pair_bits(c0n, sn, col, a.I, full, un);
        }
        cat_keep4(a, b, col, u, dr, kp);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float dz = (col + j < a.I) ? d[j] * kp[j] : 0.f;
            if constexpr (SRC == 0) {
                s0 += dz * v[j];
                s1 += dz * un[2 * j];
                s2 += dz * un[2 * j + 1];
                s3 += dz;
            } else {
#pragma clang fp contract(off)
                if (cat_grad_fused(u, j)) {
                    s0 = __builtin_fmaf(dz, v[j], s0);
                } else {
                    const float t = dz * v[j];
                    s0 = s0 + t;
                }
                const float t1 = dz * un[2 * j], t2 = dz * un[2 * j + 1];
                s1 = s1 + t1;
                s2 = s2 + t2;
                s3 = s3 + dz;
            }
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

// what the two builder entries set alike (everything but the source)
void cat_fill_prep(CatArgs& a, const int64_t* ts, const float* ca, const float* cb, int noise_mode, const float* noise, int64_t ldn,
                   int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset,
                   const float* cat_w, const float* cat_b, int E, int B, int I, float* xin, int64_t ldxin, float* xt_out,
                   int64_t ldxt) {
    a.ts = ts; a.ca = ca; a.cb = cb; a.noise_mode = ca ? noise_mode : 0;
    a.noise = noise; a.ldn = ldn;
    cat_fill_drop(a, drop_mode, keep, ldkeep, drop_p, seed, offset);
    a.cat_w = cat_w; a.cat_b = cat_b; a.B = B; a.I = I; a.one_col = (I + E < ldxin) ? I + E : -1;
    a.xin = xin; a.ldxin = ldxin; a.xt = xt_out; a.ldxt = ldxt;
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
    GD_CHECK_OFFSET(offset, "cat_prep_input");
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
    a.x = x; a.ldx = ldx; a.xU = xU; a.ldu = ldu;
    cat_fill_prep(a, ts, ca, cb, noise_mode, noise, ldn, drop_mode, keep, ldkeep, drop_p, seed, offset, cat_w, cat_b, E, B, I, xin,
                  ldxin, xt_out, ldxt);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(gd_cdiv(I, CAT_SPAN), B);
    {
        // algorithmic bytes: read x0 + the one-hot pair (+ explicit noise / keep-mask), write the item columns of xin and x_t
        const double bytes = (double)B * I * (4.0 + 8.0 + (a.noise_mode == 1 ? 4.0 : 0.0) + (drop_mode == 1 ? 1.0 : 0.0) + 8.0);
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL((cat_prep_kernel<0, CatDense>), grid, dim3(256), 0, s, a, CatDense{});
    }
    return gd_launch_status("cat_prep_input");
}

int gdmcf_cat_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts_U,
                                 float discrete, const uint8_t* sampled, int64_t lds, uint64_t offset_noise, const int64_t* ts,
                                 const float* ca, const float* cb, int noise_mode, const float* noise, int64_t ldn, int drop_mode,
                                 const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset_prep,
                                 const float* cat_w, const float* cat_b, const float* emb_w, const float* emb_b, int E, int B, int I,
                                 float* xin, int64_t ldxin, float* xt_out, int64_t ldxt, float* temb_out, uint32_t* x0bits_out,
                                 int64_t ldx0bits, uint32_t* clsbits_out, int64_t ldclsbits, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E > 0 && I <= 0x3FFFFFFF, "cat_prep_input_csr: empty batch / no embedding columns / too many items");
    GD_CHECK_SHAPE(ldxin >= (int64_t)I + E && (ldxin % 4) == 0 && gd_aligned16(xin), "cat_prep_input_csr: xin must be 16B aligned, ld%4==0, ld >= I+E");
    GD_CHECK_SHAPE(ldxt >= I && (ldxt % 4) == 0 && gd_aligned16(xt_out), "cat_prep_input_csr: x_t must be 16B aligned, ld%4==0, ld >= I");
    GD_CHECK_SHAPE(ldx0bits >= (I + 31) / 32 && ldclsbits >= (I + 31) / 32, "cat_prep_input_csr: ldx0bits / ldclsbits < ceil(I/32)");
    GD_CHECK_OFFSET(offset_noise | offset_prep, "cat_prep_input_csr");
    GD_CHECK_ARG(indptr && indices && rows, "cat_prep_input_csr: CSR arrays / row ids missing");
    GD_CHECK_ARG(xin && xt_out && x0bits_out && clsbits_out && cat_w && cat_b && ts && emb_w && emb_b, "cat_prep_input_csr: null pointer");
    GD_CHECK_ARG(sampled ? lds >= I : ts_U != nullptr, "cat_prep_input_csr: classes / ts_U missing or lds < I");
    GD_CHECK_ARG((ca == nullptr) == (cb == nullptr), "cat_prep_input_csr: ca/cb must both be set or both NULL");
    GD_CHECK_ARG(noise_mode >= 0 && noise_mode <= 2 && drop_mode >= 0 && drop_mode <= 2, "cat_prep_input_csr: bad mode");
    GD_CHECK_ARG(!ca || noise_mode != 1 || (noise && ldn >= I), "cat_prep_input_csr: explicit noise missing");
    GD_CHECK_ARG(drop_mode != 1 || (keep && ldkeep >= I), "cat_prep_input_csr: explicit keep-mask missing");
    GD_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "cat_prep_input_csr: dropout p out of range");
    // both Philox offsets are by-value arguments: this entry has no device-side step state to read them from
    GD_CHECK_ARG(t_gd_step_state == nullptr, "cat_prep_input_csr: not available while a graph step state is bound");
    int rc = gdmcf_dnn_emb_cols_f32(ts, emb_w, emb_b, E, B, I, xin, ldxin, temb_out, stream);
    if (rc) return rc;
    CatArgs a = {};
    cat_fill_prep(a, ts, ca, cb, noise_mode, noise, ldn, drop_mode, keep, ldkeep, drop_p, seed, offset_prep, cat_w, cat_b, E, B, I,
                  xin, ldxin, xt_out, ldxt);
    const CatCsr c = {indptr, indices, rows, ts_U, sampled, lds, gd_p1_off(discrete), offset_noise, x0bits_out, ldx0bits,
                      clsbits_out, ldclsbits};
    hipStream_t s = (hipStream_t)stream;
    {
        // algorithmic bytes: write the item columns of xin and x_t and the two bitmaps (+ given classes / noise / keep-mask);
        // the rows themselves are a few hundred bytes of CSR
        const double bytes = (double)B * I * ((sampled ? 1.0 : 0.0) + (a.noise_mode == 1 ? 4.0 : 0.0) + (drop_mode == 1 ? 1.0 : 0.0) + 8.0 + 0.25);
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL((cat_prep_kernel<1, CatCsr>), dim3(gd_cdiv(I, CAT_SPAN), B), dim3(256), 0, s, a, c);
    }
    return gd_launch_status("cat_prep_input_csr");
}

size_t gdmcf_cat_grad_ws_bytes(int B, int I) {
    if (B <= 0 || I <= 0) return 0;
    return (size_t)B * (size_t)gd_cdiv(I, CAT_SPAN) * 4 * sizeof(float);
}

int gdmcf_cat_grad_f32(const float* dxin, int64_t lddx, const float* xt, int64_t ldxt, const float* xU, int64_t ldu, int drop_mode,
                       const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, int B, int I, void* ws,
                       size_t ws_bytes, float* grad_w, float* grad_b, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && I <= 0x3FFFFFFF && lddx >= I && ldxt >= I && ldu >= 2 * (int64_t)I, "cat_grad: bad shape");
    GD_CHECK_OFFSET(offset, "cat_grad");
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
        hipLaunchKernelGGL((cat_grad_kernel<0, CatDense>), dim3(nbx, B), dim3(256), 0, s, a, (float*)ws, CatDense{});
    }
    hipLaunchKernelGGL(cat_grad_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, B * nbx, grad_w, grad_b);
    return gd_launch_status("cat_grad");
}

int gdmcf_cat_grad_bits_f32(const float* dxin, int64_t lddx, const float* xt, int64_t ldxt, const uint32_t* x0bits, int64_t ldx0bits,
                            const uint32_t* clsbits, int64_t ldclsbits, int drop_mode, const uint8_t* keep, int64_t ldkeep,
                            float drop_p, uint64_t seed, uint64_t offset, int B, int I, void* ws, size_t ws_bytes, float* grad_w,
                            float* grad_b, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && I <= 0x3FFFFFFF && lddx >= I && ldxt >= I, "cat_grad_bits: bad shape");
    GD_CHECK_SHAPE(ldx0bits >= (I + 31) / 32 && ldclsbits >= (I + 31) / 32, "cat_grad_bits: ldx0bits / ldclsbits < ceil(I/32)");
    GD_CHECK_OFFSET(offset, "cat_grad_bits");
    GD_CHECK_ARG(dxin && xt && x0bits && clsbits && grad_w && grad_b, "cat_grad_bits: null pointer");
    GD_CHECK_ARG(drop_mode >= 0 && drop_mode <= 2 && (drop_mode != 1 || (keep && ldkeep >= I)), "cat_grad_bits: bad mode / keep-mask missing");
    GD_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "cat_grad_bits: dropout p out of range");
    GD_CHECK_ARG(t_gd_step_state == nullptr, "cat_grad_bits: not available while a graph step state is bound");
    const int nbx = gd_cdiv(I, CAT_SPAN);
    GD_CHECK_SHAPE((int64_t)B * nbx < 2147483647LL / 4, "cat_grad_bits: too many partials");
    if (ws == nullptr || ws_bytes < gdmcf_cat_grad_ws_bytes(B, I) || !gd_aligned16(ws)) {
        gdmcf_set_error("cat_grad_bits: workspace %zu < %zu bytes (or not 16-byte aligned)", ws_bytes, gdmcf_cat_grad_ws_bytes(B, I));
        return GDMCF_E_WORKSPACE;
    }
    CatArgs a = {};
    a.xt = const_cast<float*>(xt); a.ldxt = ldxt; a.dxin = dxin; a.lddx = lddx; a.B = B; a.I = I;
    cat_fill_drop(a, drop_mode, keep, ldkeep, drop_p, seed, offset);
    const CatBits c = {x0bits, ldx0bits, clsbits, ldclsbits};
    hipStream_t s = (hipStream_t)stream;
    {
        // algorithmic bytes: read dxin, x_t and the two bitmaps (+ a given keep-mask)
        GdProfScope prof(7, (double)B * I * (4.0 + 4.0 + 0.25 + (drop_mode == 1 ? 1.0 : 0.0)), s);
        hipLaunchKernelGGL((cat_grad_kernel<1, CatBits>), dim3(nbx, B), dim3(256), 0, s, a, (float*)ws, c);
    }
    hipLaunchKernelGGL(cat_grad_reduce_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, B * nbx, grad_w, grad_b);
    return gd_launch_status("cat_grad_bits");
}

}  // extern "C"
