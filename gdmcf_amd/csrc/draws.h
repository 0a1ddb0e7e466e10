// The ONE definition of every random draw, and of the arithmetic around it, that more than one kernel must agree on bit for bit.
// Noise and dropout masks are never stored: a kernel that needs an element again (the backward pass of the cat layer, the N(0,1)
// fill handed back to the input builder as given noise, the one-hot builder that reproduces onehot_noise_kernel's classes) draws
// it again from (seed, offset, stream, position).  That only works while every such kernel evaluates the same expressions in the
// same order, so they all inline the functions below and none restates them.  Included by prep_input.hip, noise.hip, cat.hip,
// loss_tail.hip and bpr.hip -- not by common.h, which every GEMM translation unit reads.
#pragma once
#include <math.h>

#include "common.h"

// ---- streams: counter word z of Philox4x32-10 (common.h), one id per kind of draw --------------------------------------------
// counter = (position along the row, row, STREAM | (offset >> 32) << 8, (uint32)offset); the key is the seed.  Stream ids stay
// below 256 and offsets below 2^56 (GD_CHECK_OFFSET, common.h): the offset's bits 32..55 ride in word z above the stream id, so
// callers may keep disjoint draw regions apart by the offset's high bits (gaussian_diffusion.py: 1 << 40, 1 << 41, 1 << 42) and
// every draw at an offset below 2^32 has the counter (position, row, stream, offset) it always had.
enum : uint32_t {
    GD_STREAM_NOISE = 0,         // q_sample's N(0,1): prep_input.hip (xt4), cat.hip (cat_prep_kernel), randn_kernel with stream_id 0
    GD_STREAM_DROPOUT = 1,       // keep-masks: prep_input.hip, cat.hip (builder and gradient)
    GD_STREAM_TIMESTEPS = 2,     // loss_tail.hip: sample_timesteps_kernel, counter (b, 0, 2, offset)
    GD_STREAM_ONEHOT_CLASS = 3,  // noise.hip: onehot_noise_kernel; prep_input.hip: the one-hot CSR builder
    // 4: randn_kernel's default (the eps target's noise, gaussian_diffusion.py); randn_kernel takes any id below 256
    GD_STREAM_GRAPH_CLASS = 5,   // noise.hip: graph_step_kernel, the edge classes
    GD_STREAM_GRAPH_PICK = 6,    // noise.hip: graph_step_kernel, one bit per user, counter (0xFFFFFFFF, b, 6, offset)
    GD_STREAM_BPR = 7,           // bpr.hip: the triple sampler, counter (j, 0, 7, offset); also the reverse loop's randn_kernel fills
    // Triple j of the sampler owns the blocks (j, 0), (j, 1), ...: word x of block 0 draws the positive, and candidate number
    // q = k * pool + c (negative slot k, pool position c) takes word y, z, w of block 0 for q = 0, 1, 2 and word (q - 3) % 4 of
    // block (j, 1 + (q - 3) / 4) for q >= 3 (gdmcf_bpr_sample_pool_f32).  The one-negative draw of gdmcf_bpr_sample_f32 is
    // q = 0 of this layout, not a second scheme.
};

// ---- launch geometry of the builders, of randn_kernel and of the cat kernels ---------------------------------------------------
// A thread holds PREP_G column groups of four, 1024 columns apart (256 threads x 4 columns): the per-row scalars are fetched once
// per thread and a workgroup moves 16 KB in and out.  The dropout block of a PAIR of groups (below) is tied to this layout.
constexpr int PREP_G = 4;

__device__ __forceinline__ uint2 gd_philox_key(uint64_t seed) { return make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)); }
// the counter of the block of four words at position x of row b, and the block
__device__ __forceinline__ uint4 gd_counter(uint32_t x, int b, uint32_t stream, uint64_t offset) {
    return make_uint4(x, (uint32_t)b, stream | ((uint32_t)(offset >> 32) << 8), (uint32_t)offset);
}
__device__ __forceinline__ uint4 gd_philox_block(uint32_t x, int b, uint32_t stream, uint64_t offset, uint2 key) {
    return philox4x32_10(gd_counter(x, b, stream, offset), key);
}

// ---- N(0,1) ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gd_box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)a + 1.0f) * 2.3283064365386963e-10f;  // (0,1]
    const float u2 = (float)b * 2.3283064365386963e-10f;
    // hardware transcendentals (v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32 take the angle in revolutions): the libm
    // forms cost ~10x the instructions and made the input builder ALU-bound; ~1e-6 absolute error is irrelevant for
    // N(0,1) noise (tests/test_gpu_parity.py::test_philox_noise_and_dropout_statistics)
    const float rad = __builtin_amdgcn_sqrtf(-1.3862943611198906f * __builtin_amdgcn_logf(u1));  // sqrt(-2 ln u1)
    z0 = rad * __builtin_amdgcn_cosf(u2);
    z1 = rad * __builtin_amdgcn_sinf(u2);
}

// the four normals of a block: Box-Muller on (x, y) and (z, w)
__device__ __forceinline__ void gd_block_normals(const uint4& r, float (&z)[4]) {
    gd_box_muller(r.x, r.y, z[0], z[1]);
    gd_box_muller(r.z, r.w, z[2], z[3]);
}

// the normals of columns col .. col + 3 (col a multiple of 4) of row b: element i of a row is normal i & 3 of the block at
// position i >> 2, counter gd_normal_counter
__device__ __forceinline__ uint4 gd_normal_counter(int col, int b, uint32_t stream, uint64_t offset) {
    return gd_counter((uint32_t)(col >> 2), b, stream, offset);
}
__device__ __forceinline__ void gd_normal4(int col, int b, uint32_t stream, uint64_t offset, uint2 key, float (&z)[4]) {
    gd_block_normals(philox4x32_10(gd_normal_counter(col, b, stream, offset), key), z);
}

// q_sample (reference gaussian_diffusion.py:403-407): two rounded products + one rounded sum, exactly as the reference's mul, mul,
// add: no FMA contraction here (HIP's __fmul_rn/__fadd_rn are plain operators and would still fuse)
__device__ __forceinline__ float gd_qsample(float ca, float x, float cb, float n) {
#pragma clang fp contract(off)
    const float p0 = ca * x;
    const float p1 = cb * n;
    return p0 + p1;
}

// ---- class draws of the discrete transition noise (reference gaussian_diffusion.py:770-831, :706-729) ---------------------------
// uniform in [0, 1) from the top 24 bits of a word
__device__ __forceinline__ float gd_uniform24(uint32_t u) { return (float)(u >> 8) * 5.9604644775390625e-8f; }

// the class drawn for an item of class c from row c of Q = a*I + (1-a)*[[e,1-e],[e,1-e]]:
// P(class 1) = a*[c == 1] + (1 - a)*(1 - e), each product and the sum rounded to f32 as torch does.
// a = gd_class_scale(ts[b], B), p1_off = gd_p1_off(e).
__device__ __forceinline__ int gd_class_draw(int c, float a, float p1_off, uint32_t u) {
    float p1;
    {
#pragma clang fp contract(off)
        const float q = (1.f - a) * p1_off;
        p1 = (c ? a : 0.f) + q;
    }
    return gd_uniform24(u) < p1;
}
// a = (float)ts[b] / B (the reference's own scaling, :775)
__device__ __forceinline__ float gd_class_scale(int64_t t, int B) { return __fdiv_rn((float)t, (float)B); }
// u_x = th.tensor([[e, 1 - e], ...]): 1 - e is formed in double and rounded to float32 once
static inline float gd_p1_off(float discrete) { return (float)(1.0 - (double)discrete); }

// ---- dropout --------------------------------------------------------------------------------------------------------------
// keep iff (16-bit uniform) < thresh = round((1 - p) * 65536): the keep probability is quantised to 2^-16 (exact for p = 0.5);
// scale = 1/(1-p)
static inline void gd_drop_params(float p, float* scale, uint32_t* thresh) {
    *scale = 1.0f / (1.0f - p);
    *thresh = (uint32_t)fmin(fmax(rint((1.0 - (double)p) * 65536.0), 0.0), 65536.0);
}

// ONE block gives the 16-bit uniforms of a PAIR of a thread's column groups (u, u + 1), u even: counter
// ((col of the even group) >> 2, b, 1, offset); the even group takes the low 16 bits of each word, the odd group (odd = 1)
// the high 16.  (odd = u & 1 is the caller's: the builder's rolled tail pass also steps back to the even group's column with it.)
__device__ __forceinline__ uint4 gd_drop_block(int col_even_group, int b, uint64_t offset, uint2 key) {
    return gd_philox_block((uint32_t)(col_even_group >> 2), b, GD_STREAM_DROPOUT, offset, key);
}
__device__ __forceinline__ void gd_drop_bits(const uint4& block, int odd, uint32_t (&du)[4]) {
    const int dsh = 16 * odd;
    du[0] = (block.x >> dsh) & 0xFFFFu; du[1] = (block.y >> dsh) & 0xFFFFu;
    du[2] = (block.z >> dsh) & 0xFFFFu; du[3] = (block.w >> dsh) & 0xFFFFu;
}

// ---- row access (f32x4_u4, common.h: rows of a dense batch are only 4-byte aligned when the width is odd) ------------------------
// four consecutive values of a row from column col: one 16-byte load when all four exist (`full`), else element-wise (0 behind n)
__device__ __forceinline__ void gd_load4(const float* row, int col, int n, bool full, float (&v)[4]) {
    if (full) {
        const f32x4 t = *reinterpret_cast<const f32x4_u4*>(row + col);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (col + j < n) ? row[col + j] : 0.f;
    }
}

// the same into an array the caller has zeroed: the ragged branch writes only the elements that exist
__device__ __forceinline__ void gd_load4_zeroed(const float* row, int col, int n, bool full, float (&v)[4]) {
    if (full) {
        const f32x4 t = *reinterpret_cast<const f32x4_u4*>(row + col);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (col + j < n) v[j] = row[col + j];
    }
}
