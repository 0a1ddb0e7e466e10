// The denoiser-input builder: q_sample + F.normalize + dropout + timestep embedding + cat in one pass, from dense rows, from CSR
// rows, or from the one-hot image of CSR rows under the discrete transition noise.  Belongs here: PrepArgs / OneHotSrc, the
// builder's body and its kernels, the embedding-column kernel (the owner of that part of xin's layout, also launched by cat.hip's
// entry), and their C entries.  Every draw and every rounding another kernel has to reproduce comes from draws.h.
#include "draws.h"

namespace {

struct PrepArgs {
    const float* x;
    int64_t ldx;
    const int64_t* ts;
    const float* ca;
    const float* cb;
    int noise_mode;
    const float* noise;
    int64_t ldn;
    int drop_mode;
    const uint8_t* keep;
    int64_t ldkeep;
    float drop_scale;      // 1/(1-p)
    uint32_t keep_thresh;  // keep iff (16-bit uniform) < keep_thresh (draws.h: gd_drop_params)
    uint64_t seed, offset;
    const GdStepState* step_state;  // graph mode: the Philox offset is read from the device (NULL: `offset`)
    const float* rownorm;  // [B] L2 norms of x_t rows (normalize) or NULL
    const float* emb_w;
    const float* emb_b;
    int E, B, I;
    float* xin;
    int64_t ldxin;
    float* xt_out;
    int64_t ldxt;
    float* temb_out;
    unsigned short* xin16;  // bf16 shadow of xin (or NULL), row stride ldxin16 (a multiple of 64 >= I+E)
    int64_t ldxin16;
    // CSR source (gdmcf_dnn_prep_input_csr_f32): row b of the batch is row csr_rows[b] of a {0,1} matrix held as CSR;
    // x is NULL then.  bits_out receives the rows as bitmaps (word w of row b = columns 32w .. 32w+31), the loss target.
    const int64_t* csr_indptr;
    const int32_t* csr_indices;
    const int64_t* csr_rows;
    uint32_t* bits_out;
    int64_t ldbits;
};

// (out of line: a few hundred threads of a launch evaluate it, but inlined its libm sinusoids -- Payne-Hanek reductions and all --
// were two thirds of the input builder's 8 500 lines of ISA and cost the hot loop ~3.5 us of instruction fetch,
// profiles/r04_prep_input_ablation.txt)
__device__ __noinline__ float temb_value(float t, int f, int E) {
    // reference models/DNN.py:1817-1825: [cos(t*freqs), sin(t*freqs), (0 if E odd)]
    const int half = E / 2;
    if (f >= 2 * half) return 0.f;
    const int j = (f < half) ? f : f - half;
    const float freq = expf(-9.210340371976184f * (float)j / (float)half);
    const float a = t * freq;
    return (f < half) ? cosf(a) : sinf(a);
}

// x_t for 4 consecutive columns of one row (shared by the row-norm pass and the main pass)
template <bool FULL = false>  // FULL: the caller knows col + 3 < I (no per-element bounds checks)
__device__ __forceinline__ void xt4(const PrepArgs& a, int b, int col, float ca, float cb, float (&v)[4],
                                    const uint32_t* bm = nullptr, int bm_col0 = 0) {
    const float* xr = a.x + (int64_t)b * a.ldx;
    const bool full = FULL || col + 3 < a.I;
    if (bm) {  // CSR source: the workgroup's span as a bitmap in LDS (col is a multiple of 4: one word holds all four)
        const uint32_t w = bm[(col - bm_col0) >> 5] >> ((col - bm_col0) & 31);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((FULL || col + j < a.I) && ((w >> j) & 1u)) ? 1.f : 0.f;
    } else {
        gd_load4(xr, col, a.I, full, v);
    }
    if (a.ca) {
        float nz[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.noise_mode == 1)
            gd_load4_zeroed(a.noise + (int64_t)b * a.ldn, col, a.I, full, nz);
        else if (a.noise_mode == 2)
            gd_normal4(col, b, GD_STREAM_NOISE, a.offset, gd_philox_key(a.seed), nz);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = gd_qsample(ca, v[j], cb, nz[j]);
    }
}

// One-hot CSR source (gdmcf_onehot_prep_input_csr_f32): the builder's "row" is the [2I] one-hot image of a {0,1} CSR row under the
// discrete transition noise of onehot_noise_kernel -- columns (2i, 2i + 1) of item i -- formed on the fly: no dense row, no xU.
struct OneHotSrc {
    const int64_t* ts_U;   // [B] timesteps of the class draws (may be NULL when the classes are given)
    const uint8_t* sampled;  // given classes [B, lds] or NULL: drawn (stream 3, `offset`)
    int64_t lds;
    uint8_t* sampled_out;  // optional [B, ldso]
    int64_t ldso;
    float p1_off;     // (float)(1 - e)
    uint64_t offset;  // Philox offset of the class draws (the builder's own `PrepArgs::offset` is the dropout's)
    int items;        // I (PrepArgs::I is 2I here)
};

// the two class uniforms of the items (col >> 1, (col >> 1) + 1) behind a group of four one-hot columns: words (0, 1) or (2, 3)
// -- by (col >> 2) & 1 -- of the stream-3 block onehot_noise_kernel draws for the four items (col >> 3) * 4 ..
__device__ __forceinline__ void onehot_uniforms(const PrepArgs& a, const OneHotSrc& o, int b, int col, uint32_t (&u)[2]) {
    const uint4 r = gd_philox_block((uint32_t)(col >> 3), b, GD_STREAM_ONEHOT_CLASS, o.offset, gd_philox_key(a.seed));
    const bool hi = (col >> 2) & 1;
    u[0] = hi ? r.z : r.x;
    u[1] = hi ? r.w : r.y;
}

// the four one-hot columns col .. col + 3 of row b: exactly what onehot_noise_kernel writes to xU[b, col .. col + 3] (same
// `a`, same gd_class_draw).  bm: the workgroup's 2048 items as bits; u: onehot_uniforms (drawn classes).
template <bool FULL>
__device__ __forceinline__ void onehot4(const PrepArgs& a, const OneHotSrc& o, int b, int col, float an, const uint32_t (&u)[2],
                                        float (&v)[4], const uint32_t* bm, int bm_col0) {
    const int it = (col - bm_col0) >> 1;  // even: both items' bits sit in one word
    const uint32_t w = bm[it >> 5] >> (it & 31);
    const int i0 = col >> 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const bool in = FULL || col + 2 * j < a.I;
        const int c0 = in && ((w >> j) & 1u);
        int s = 0;
        if (o.sampled) {
            if (in) s = o.sampled[(int64_t)b * o.lds + i0 + j] != 0;
        } else {
            s = gd_class_draw(c0, an, o.p1_off, u[j]);
        }
        if (o.sampled_out && in) o.sampled_out[(int64_t)b * o.ldso + i0 + j] = (uint8_t)s;
        const float keep = (in && s == c0) ? 1.f : 0.f;
        v[2 * j] = c0 ? 0.f : keep;
        v[2 * j + 1] = c0 ? keep : 0.f;
    }
}

__global__ __launch_bounds__(256) void prep_rowss_kernel(PrepArgs a, float* __restrict__ rownorm) {
    if (a.step_state) a.offset = a.step_state->prep_offset;
    const int b = blockIdx.x;
    float ca = 1.f, cb = 0.f;
    if (a.ca) {
        const int64_t t = a.ts[b];
        ca = a.ca[t];
        cb = a.cb[t];
    }
    float ss = 0.f;
    for (int col = threadIdx.x * 4; col < a.I; col += 256 * 4) {
        float v[4];
        xt4(a, b, col, ca, cb, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j < a.I) ss += v[j] * v[j];  // (in-kernel noise draws all four normals of a ragged group: x_t past I is not 0)
    }
    __shared__ float red[4];
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) rownorm[b] = sqrtf(red[0] + red[1] + red[2] + red[3]);
}

// SRC 0: dense rows / CSR rows (prep_input_kernel).  SRC 1: the one-hot image of CSR rows (onehot_prep_input_csr_kernel) -- a
// compile-time source, so that the SRC 0 kernel's ISA is what it was (the builder is instruction-fetch- and VALU-issue-bound,
// profiles/r04_prep_input_ablation.txt); dropout, embedding columns, the 1 behind them and the padding are this one body.
template <int SRC>
__device__ __forceinline__ void prep_input_body(PrepArgs a, const OneHotSrc o) {
    if (SRC == 0 && a.step_state) a.offset = a.step_state->prep_offset;
    const int b = blockIdx.y;
    const int64_t t = a.ts ? a.ts[b] : 0;
    float ca = 1.f, cb = 0.f;
    if (a.ca) {
        ca = a.ca[t];
        cb = a.cb[t];
    }
    // the workgroup that holds the embedding columns evaluates the E sinusoids ONCE, one per lane, instead of E times
    // per embedding column in a serial chain of libm calls (that chain was a ~15 us tail of the whole launch)
    __shared__ float s_temb[256];
    __shared__ uint32_t s_bm[256 * PREP_G * 4 / 32];  // CSR source: this workgroup's 4096 columns of row b as bits
    const int bm_col0 = blockIdx.x * (256 * PREP_G * 4);
    if (SRC == 1 || a.csr_indptr) {
        // CSR source: the row's entries inside the workgroup's span, marked as bits (SRC 1: its 4096 one-hot columns are 2048 items)
        constexpr int SPAN = 256 * PREP_G * (SRC == 1 ? 2 : 4);
        const int first = SRC == 1 ? bm_col0 >> 1 : bm_col0;
        if (threadIdx.x < SPAN / 32) s_bm[threadIdx.x] = 0u;
        __syncthreads();
        const int64_t r = a.csr_rows[b];
        const int64_t beg = a.csr_indptr[r], end = a.csr_indptr[r + 1];
        for (int64_t k = beg + threadIdx.x; k < end; k += 256) {
            const int ci = a.csr_indices[k];
            const int c = ci - first;
            if (c >= 0 && c < SPAN && ci < (SRC == 1 ? o.items : a.I)) atomicOr(&s_bm[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
        if (a.bits_out && threadIdx.x < SPAN / 32) {
            const int64_t w = (int64_t)(first >> 5) + threadIdx.x;
            if (w < a.ldbits) a.bits_out[(int64_t)b * a.ldbits + w] = s_bm[threadIdx.x];
        }
    }
    const uint32_t* bm = (SRC == 1 || a.csr_indptr) ? s_bm : nullptr;
    const bool has_emb = a.E > 0 && a.E <= 256 && (int)((blockIdx.x + 1) * (256 * PREP_G * 4)) > a.I;
    if (has_emb) {
        if ((int)threadIdx.x < a.E) s_temb[threadIdx.x] = temb_value((float)t, threadIdx.x, a.E);
        __syncthreads();
    }
    const uint2 key = gd_philox_key(a.seed);
    const int col_base = (blockIdx.x * (256 * PREP_G) + threadIdx.x) * 4;  // group u of this thread: col_base + 1024 u
    // ---- the hot path: whole groups of four item columns (all but the last group or two of a row) ----
    uint4 dr = make_uint4(0u, 0u, 0u, 0u);  // dropout uniforms of a PAIR of column groups (u, u + 1): 16 bits per element
    // SRC 1, drawn classes.  A group of four columns is two items: half a stream-3 block, whose other half belongs to the
    // neighbouring lane's group (lanes 2k and 2k + 1 hold the columns of the four items of one block, for every u).  The block
    // is SHARED, not computed twice: of the pair's PREP_G blocks the even lane computes those of u = 0, 1 and the odd lane
    // those of u = 2, 3, and each hands the other the half it needs with one lane swap per word (own[k] / got[k]: block of
    // u = 2 * parity + k resp. u = 2 * (1 - parity) + k).  That keeps the builder at PREP_G / 2 class blocks + PREP_G / 2 dropout
    // blocks per thread -- what onehot_noise_kernel plus the dense builder spend per four columns -- where the straightforward
    // form doubles the class blocks (+ 50 % Philox in a VALU-issue-bound kernel).  All lanes of the workgroup get here (no
    // divergence before the swaps); the rolled tail pass below, which is divergent, draws its own block instead.
    uint32_t own[PREP_G / 2][2] = {}, got[PREP_G / 2][2] = {};
    float an = 1.f;
    const int par = threadIdx.x & 1;
    if (SRC == 1 && !o.sampled) {
        an = gd_class_scale(o.ts_U[b], a.B);
#pragma unroll
        for (int k = 0; k < PREP_G / 2; ++k) {
            const int colk = col_base + (2 * par + k) * 1024;
            const uint4 r = gd_philox_block((uint32_t)(colk >> 3), b, GD_STREAM_ONEHOT_CLASS, o.offset, key);
            own[k][0] = par ? r.z : r.x;
            own[k][1] = par ? r.w : r.y;
            got[k][0] = __shfl_xor(par ? r.x : r.z, 1);
            got[k][1] = __shfl_xor(par ? r.y : r.w, 1);
        }
    }
#pragma unroll
    for (int u = 0; u < PREP_G; ++u) {
        const int col = col_base + u * 1024;
        if (a.drop_mode == 2 && (u & 1) == 0 && col < a.I) dr = gd_drop_block(col, b, a.offset, key);
        if (col + 3 >= a.I) continue;  // (the tail pass below)
        uint32_t du[4];
        gd_drop_bits(dr, u & 1, du);
        float v[4];
        if (SRC == 1) {
            const bool mine = par == (u >> 1);
            const uint32_t cu[2] = {mine ? own[u & 1][0] : got[u & 1][0], mine ? own[u & 1][1] : got[u & 1][1]};
            onehot4<true>(a, o, b, col, an, cu, v, bm, bm_col0);
        } else {
            xt4<true>(a, b, col, ca, cb, v, bm, bm_col0);
        }
        if (SRC == 0 && a.xt_out) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a.xt_out[(int64_t)b * a.ldxt + col + j] = v[j];
        }
        if (SRC == 0 && a.rownorm) {
            const float dn = fmaxf(a.rownorm[b], 1e-12f);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = v[j] / dn;
        }
        if (a.drop_mode == 1) {
            const uint8_t* kr = a.keep + (int64_t)b * a.ldkeep + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = kr[j] ? v[j] * a.drop_scale : 0.f;
        } else if (a.drop_mode == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (du[j] < a.keep_thresh) ? v[j] * a.drop_scale : 0.f;
        }
        *reinterpret_cast<f32x4*>(a.xin + (int64_t)b * a.ldxin + col) = f32x4{v[0], v[1], v[2], v[3]};
        if (a.xin16 && col < a.ldxin16) {
            const uint2 w = make_uint2(gd_bf16_bits(v[0]) | ((unsigned)gd_bf16_bits(v[1]) << 16),
                                       gd_bf16_bits(v[2]) | ((unsigned)gd_bf16_bits(v[3]) << 16));
            *reinterpret_cast<uint2*>(a.xin16 + (int64_t)b * a.ldxin16 + col) = w;
        }
    }
    // ---- the tail pass: the row's last (ragged) item group, the timestep-embedding columns [I, I+E) and the zero padding up to
    // ldxin -- a few dozen groups of a row, ONE rolled instance of the code (unrolled beside the hot path it was most of the
    // kernel's 8 500 lines of ISA: ~3.5 us of instruction fetch, profiles/r04_prep_input_ablation.txt) ----
#pragma unroll 1
    for (int u = 0; u < PREP_G; ++u) {
        const int col = col_base + u * 1024;
        if (col + 3 < a.I || col >= a.ldxin) continue;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (col < a.I) {
            if (SRC == 1) {
                uint32_t cu[2] = {0u, 0u};
                if (!o.sampled) onehot_uniforms(a, o, b, col, cu);
                onehot4<false>(a, o, b, col, an, cu, v, bm, bm_col0);
            } else {
                xt4(a, b, col, ca, cb, v, bm, bm_col0);
            }
            if (SRC == 0 && a.xt_out) {
                for (int j = 0; j < 4; ++j)
                    if (col + j < a.I) a.xt_out[(int64_t)b * a.ldxt + col + j] = v[j];
            }
            if (SRC == 0 && a.rownorm) {
                const float dn = fmaxf(a.rownorm[b], 1e-12f);
                for (int j = 0; j < 4; ++j) v[j] = v[j] / dn;
            }
            if (a.drop_mode == 1) {
                const uint8_t* kr = a.keep + (int64_t)b * a.ldkeep;
                for (int j = 0; j < 4; ++j)
                    if (col + j < a.I) v[j] = kr[col + j] ? v[j] * a.drop_scale : 0.f;
            } else if (a.drop_mode == 2) {  // the pair's block again (same counter as in the hot path: group u & ~1 of this thread)
                const int odd = u & 1;
                uint32_t du[4];
                gd_drop_bits(gd_drop_block(col - odd * 1024, b, a.offset, key), odd, du);
                for (int j = 0; j < 4; ++j) v[j] = (du[j] < a.keep_thresh) ? v[j] * a.drop_scale : 0.f;
            }
        }
        for (int j = 0; j < 4; ++j) {
            const int i = col + j;
            if (i >= a.I) {
                float e = 0.f;
                if (i < a.I + a.E) {
                    const int eo = i - a.I;
                    e = a.emb_b[eo];
                    for (int f = 0; f < a.E; ++f) e += a.emb_w[eo * a.E + f] * (has_emb ? s_temb[f] : temb_value((float)t, f, a.E));
                    if (a.temb_out) a.temb_out[(int64_t)b * a.E + eo] = has_emb ? s_temb[eo] : temb_value((float)t, eo, a.E);
                }
                v[j] = e;
            }
        }
        *reinterpret_cast<f32x4*>(a.xin + (int64_t)b * a.ldxin + col) = f32x4{v[0], v[1], v[2], v[3]};
        if (a.xin16 && col < a.ldxin16) {
            const uint2 w = make_uint2(gd_bf16_bits(v[0]) | ((unsigned)gd_bf16_bits(v[1]) << 16),
                                       gd_bf16_bits(v[2]) | ((unsigned)gd_bf16_bits(v[3]) << 16));
            *reinterpret_cast<uint2*>(a.xin16 + (int64_t)b * a.ldxin16 + col) = w;
        }
        // column I + E of the float32 matrix (the first padding column, when there is one) holds 1: as one more column of the first
        // layer's weight-gradient product's operand it makes that layer's bias gradient a column of the product
        // (gdmcf_linear_bwd_weight_f32, a_scale_col).  The bf16 shadow keeps its zero there.  (Same thread, same address, program order.)
        const int oc = a.I + a.E;
        if (oc < a.ldxin && col <= oc && oc < col + 4) a.xin[(int64_t)b * a.ldxin + oc] = 1.f;
    }
}

__global__ __launch_bounds__(256) void prep_input_kernel(PrepArgs a) { prep_input_body<0>(a, OneHotSrc{}); }

__global__ __launch_bounds__(256) void onehot_prep_input_csr_kernel(PrepArgs a, OneHotSrc o) { prep_input_body<1>(a, o); }

__global__ void emb_cols_kernel(const int64_t* __restrict__ ts, const float* __restrict__ emb_w,
                                const float* __restrict__ emb_b, int E, int I, float* __restrict__ xin, int64_t ldxin,
                                float* __restrict__ temb_out, unsigned short* __restrict__ xin16, int64_t ldxin16) {
    const int b = blockIdx.x;
    const float t = (float)ts[b];
    // the E sinusoids once per row, one per lane (not E + 1 of them in a serial chain of libm calls per embedding column)
    __shared__ float s_temb[256];
    const bool staged = E <= 256;
    if (staged) {
        for (int f = threadIdx.x; f < E; f += blockDim.x) s_temb[f] = temb_value(t, f, E);
        __syncthreads();
    }
    for (int i = I + threadIdx.x; i < ldxin; i += blockDim.x) {
        float e = 0.f;
        if (i < I + E) {
            const int eo = i - I;
            e = emb_b[eo];
            for (int f = 0; f < E; ++f) e += emb_w[eo * E + f] * (staged ? s_temb[f] : temb_value(t, f, E));
            if (temb_out) temb_out[(int64_t)b * E + eo] = staged ? s_temb[eo] : temb_value(t, eo, E);
        }
        xin[(int64_t)b * ldxin + i] = e;
        if (xin16 && i < ldxin16) xin16[(int64_t)b * ldxin16 + i] = gd_bf16_bits(e);
    }
}

// What the three builder entries share: the argument checks behind each entry's own shape checks (`who`: the entry's message
// prefix) and every field of PrepArgs they set alike, the dropout parameters and the bf16 shadow of xin among them.  width: the
// builder's row width (I, or 2I for the one-hot image).  Left to the entry: the source (x / CSR), step_state, xt_out, OneHotSrc.
int prep_args_common(PrepArgs& a, const char* who, const int64_t* ts, const float* ca, const float* cb, int noise_mode,
                     const float* noise, int64_t ldn, int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p,
                     uint64_t seed, uint64_t offset, const float* emb_w, const float* emb_b, int E, int B, int width, float* xin,
                     int64_t ldxin, float* temb_out) {
    const char* bad = nullptr;
    if ((ca == nullptr) != (cb == nullptr)) bad = "ca/cb must both be set or both NULL";
    else if (noise_mode < 0 || noise_mode > 2 || drop_mode < 0 || drop_mode > 2) bad = "bad mode";
    else if (noise_mode == 1 && !(noise && ldn >= width)) bad = "explicit noise missing";
    else if (drop_mode == 1 && !(keep && ldkeep >= width)) bad = "explicit keep-mask missing";
    else if (!(drop_p >= 0.f && drop_p < 1.f)) bad = "dropout p out of range";
    else if (E != 0 && !(emb_w && emb_b && ts)) bad = "embedding weights / ts missing";
    else if (ca && !ts) bad = "ts missing";
    if (bad) {
        gdmcf_set_error("%s: %s", who, bad);
        return GDMCF_E_ARG;
    }
    a = PrepArgs{};
    a.ts = ts; a.ca = ca; a.cb = cb; a.noise_mode = ca ? noise_mode : 0; a.noise = noise; a.ldn = ldn;
    a.drop_mode = drop_mode; a.keep = keep; a.ldkeep = ldkeep;
    gd_drop_params(drop_p, &a.drop_scale, &a.keep_thresh);
    a.seed = seed; a.offset = offset; a.emb_w = emb_w; a.emb_b = emb_b; a.E = E; a.B = B; a.I = width;
    a.xin = xin; a.ldxin = ldxin; a.temb_out = temb_out;
    GdShadow sh;
    if (gd_shadow_lookup(xin, &sh) && sh.rows == B && sh.cols == width + E) {  // keep the bf16 shadow of xin in sync
        a.xin16 = (unsigned short*)sh.p16;
        a.ldxin16 = sh.ld16;
    }
    return GDMCF_OK;
}

dim3 prep_grid(int64_t ldxin, int B) { return dim3(gd_cdiv((int)(ldxin / 4), 256 * PREP_G), B); }

}  // namespace

extern "C" {

int gdmcf_dnn_prep_input_f32(const float* x, int64_t ldx, const int64_t* ts, const float* ca, const float* cb,
                             int noise_mode, const float* noise, int64_t ldn, int drop_mode, const uint8_t* keep,
                             int64_t ldkeep, float drop_p, uint64_t seed, uint64_t offset, int normalize,
                             const float* emb_w, const float* emb_b, int E, int B, int I, float* xin, int64_t ldxin,
                             float* xt_out, int64_t ldxt, float* temb_out, float* rownorm_ws, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E >= 0, "prep_input: empty batch");
    GD_CHECK_SHAPE(ldxin >= I + E && (ldxin % 4) == 0 && gd_aligned16(xin), "prep_input: xin must be 16B aligned, ld%4==0");
    GD_CHECK_SHAPE(ldx >= I, "prep_input: ldx < I");
    GD_CHECK_OFFSET(offset, "prep_input");
    PrepArgs a;
    const int rc = prep_args_common(a, "prep_input", ts, ca, cb, noise_mode, noise, ldn, drop_mode, keep, ldkeep, drop_p, seed,
                                    offset, emb_w, emb_b, E, B, I, xin, ldxin, temb_out);
    if (rc) return rc;
    a.x = x; a.ldx = ldx; a.step_state = t_gd_step_state; a.xt_out = xt_out; a.ldxt = ldxt;
    hipStream_t s = (hipStream_t)stream;
    if (normalize) {
        // F.normalize (reference models/DNN.py:75-76) needs the L2 norm of the noised row first
        GD_CHECK_ARG(rownorm_ws != nullptr, "prep_input: normalize needs rownorm_ws [B]");
        hipLaunchKernelGGL(prep_rowss_kernel, dim3(B), dim3(256), 0, s, a, rownorm_ws);
        a.rownorm = rownorm_ws;
    }
    {
        // algorithmic bytes: read x (+ explicit noise / keep-mask), write xin
        const double bytes = (double)B * I * (4.0 + (a.noise_mode == 1 ? 4.0 : 0.0) + (drop_mode == 1 ? 1.0 : 0.0)) +
                             (double)B * ldxin * 4.0;
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL(prep_input_kernel, prep_grid(ldxin, B), dim3(256), 0, s, a);
    }
    return gd_launch_status("prep_input");
}

int gdmcf_dnn_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts,
                                 const float* ca, const float* cb, int noise_mode, const float* noise, int64_t ldn,
                                 int drop_mode, const uint8_t* keep, int64_t ldkeep, float drop_p, uint64_t seed,
                                 uint64_t offset, const float* emb_w, const float* emb_b, int E, int B, int I, float* xin,
                                 int64_t ldxin, float* temb_out, uint32_t* bits_out, int64_t ldbits, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E >= 0, "prep_input_csr: empty batch");
    GD_CHECK_SHAPE(ldxin >= I + E && (ldxin % 4) == 0 && gd_aligned16(xin), "prep_input_csr: xin must be 16B aligned, ld%4==0");
    GD_CHECK_OFFSET(offset, "prep_input_csr");
    GD_CHECK_ARG(indptr && indices && rows, "prep_input_csr: CSR arrays / row ids missing");
    GD_CHECK_ARG(!bits_out || ldbits >= (I + 31) / 32, "prep_input_csr: ldbits < ceil(I/32)");
    PrepArgs a;
    const int rc = prep_args_common(a, "prep_input_csr", ts, ca, cb, noise_mode, noise, ldn, drop_mode, keep, ldkeep, drop_p, seed,
                                    offset, emb_w, emb_b, E, B, I, xin, ldxin, temb_out);
    if (rc) return rc;
    a.step_state = t_gd_step_state; a.csr_indptr = indptr; a.csr_indices = indices; a.csr_rows = rows; a.bits_out = bits_out; a.ldbits = ldbits;
    hipStream_t s = (hipStream_t)stream;
    {
        // algorithmic bytes: write xin (+ explicit noise / keep-mask); the rows themselves are a few hundred bytes of CSR
        const double bytes = (double)B * I * ((a.noise_mode == 1 ? 4.0 : 0.0) + (drop_mode == 1 ? 1.0 : 0.0)) +
                             (double)B * ldxin * 4.0;
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL(prep_input_kernel, prep_grid(ldxin, B), dim3(256), 0, s, a);
    }
    return gd_launch_status("prep_input_csr");
}

int gdmcf_onehot_prep_input_csr_f32(const int64_t* indptr, const int32_t* indices, const int64_t* rows, const int64_t* ts_U,
                                    float discrete, const uint8_t* sampled, int64_t lds, uint64_t seed, uint64_t offset_noise,
                                    uint8_t* sampled_out, int64_t ldso, const int64_t* ts, int drop_mode, const uint8_t* keep,
                                    int64_t ldkeep, float drop_p, uint64_t offset_prep, const float* emb_w, const float* emb_b,
                                    int E, int B, int I, float* xin, int64_t ldxin, float* temb_out, uint32_t* bits_out,
                                    int64_t ldbits, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E >= 0 && I <= 0x3FFFFFFF, "onehot_prep_input_csr: empty batch / too many items");
    const int I2 = 2 * I;
    GD_CHECK_SHAPE(ldxin >= (int64_t)I2 + E && (ldxin % 4) == 0 && gd_aligned16(xin),
                   "onehot_prep_input_csr: xin must be 16B aligned, ld%4==0, ld >= 2I+E");
    GD_CHECK_OFFSET(offset_noise | offset_prep, "onehot_prep_input_csr");
    GD_CHECK_ARG(indptr && indices && rows, "onehot_prep_input_csr: CSR arrays / row ids missing");
    GD_CHECK_ARG(!bits_out || ldbits >= (I + 31) / 32, "onehot_prep_input_csr: ldbits < ceil(I/32)");
    GD_CHECK_ARG((sampled ? lds >= I : ts_U != nullptr) && (!sampled_out || ldso >= I),
                 "onehot_prep_input_csr: classes / ts_U missing or bad leading dimension");
    PrepArgs a;  // (no q_sample here: the builder's row is the one-hot image, its noise the class draws of OneHotSrc)
    const int rc = prep_args_common(a, "onehot_prep_input_csr", ts, nullptr, nullptr, 0, nullptr, 0, drop_mode, keep, ldkeep,
                                    drop_p, seed, offset_prep, emb_w, emb_b, E, B, I2, xin, ldxin, temb_out);
    if (rc) return rc;
    // both Philox offsets are by-value arguments: this entry has no device-side step state to read them from
    GD_CHECK_ARG(t_gd_step_state == nullptr, "onehot_prep_input_csr: not available while a graph step state is bound");
    a.csr_indptr = indptr; a.csr_indices = indices; a.csr_rows = rows; a.bits_out = bits_out; a.ldbits = ldbits;
    const OneHotSrc o = {ts_U, sampled, lds, sampled_out, ldso, gd_p1_off(discrete), offset_noise, I};
    hipStream_t s = (hipStream_t)stream;
    {
        // algorithmic bytes: write xin (+ given classes / keep-mask, the classes written back); the rows are a few hundred bytes of CSR
        const double bytes = (double)B * I * ((sampled ? 1.0 : 0.0) + (sampled_out ? 1.0 : 0.0) + (drop_mode == 1 ? 2.0 : 0.0)) +
                             (double)B * ldxin * 4.0;
        GdProfScope prof(7, bytes, s);
        hipLaunchKernelGGL(onehot_prep_input_csr_kernel, prep_grid(ldxin, B), dim3(256), 0, s, a, o);
    }
    return gd_launch_status("onehot_prep_input_csr");
}

int gdmcf_dnn_emb_cols_f32(const int64_t* ts, const float* emb_w, const float* emb_b, int E, int B, int I, float* xin,
                           int64_t ldxin, float* temb_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && E > 0 && ldxin >= I + E, "emb_cols: bad shape");
    GdShadow sh;
    const bool has16 = gd_shadow_lookup(xin, &sh) && sh.rows == B && sh.cols == I + E;
    hipLaunchKernelGGL(emb_cols_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ts, emb_w, emb_b, E, I, xin, ldxin,
                       temb_out, has16 ? (unsigned short*)sh.p16 : nullptr, has16 ? sh.ld16 : 0);
    return gd_launch_status("emb_cols");
}

}  // extern "C"
