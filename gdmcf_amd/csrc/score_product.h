// The product step the fused LightGCN ranking kernels share (score_topk.hip: selection; score_rank.hip: counting, and the scores of
// the named targets): score(row, item) = dot(user row, item row) by a chain of v_mfma_f32_16x16x4_f32 from +0.  A wave multiplies
// 16 RB user rows (A: row rb*16 + (lane & 15)) by 16 item rows (B: item lane & 15); lane group lg = lane >> 4 holds the k's
// 16 j + 4 lg + s of fragment j, and the chain runs j ascending, s = 0..3 inside: the MFMA of (j, s) adds the four products
// k = 16 j + s + 4 lg', lg' = 0..3.  An output element depends on nothing but its own A row, its own B column and this order, so
// two kernels that run this text give one (row, item) the same bits wherever they seat it.  Rows are zero-padded past d.
#pragma once
#include "common.h"

namespace {

constexpr int SP_STEP = 64;  // items per workgroup step (4 waves x 16)

// four consecutive floats of a table row, zero past d; `vec`: rows are 16-byte aligned and d % 4 == 0
__device__ __forceinline__ f32x4 sp_load4(const float* __restrict__ row, int k0, int d, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
        if (k0 < d) v = *reinterpret_cast<const f32x4*>(row + k0);
    } else {
        if (k0 < d) v.x = row[k0];
        if (k0 + 1 < d) v.y = row[k0 + 1];
        if (k0 + 2 < d) v.z = row[k0 + 2];
        if (k0 + 3 < d) v.w = row[k0 + 3];
    }
    return v;
}

// the four fragments of a row with d <= 64: what a lane keeps in registers of a user row (AREG) or requests of the next item
__device__ __forceinline__ void sp_load_frags(f32x4 (&f)[4], const float* __restrict__ row, int lg, int d, bool vec) {
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = sp_load4(row, 16 * j + 4 * lg, d, vec);
}

// d <= 64, both operands in registers
template <int RB>
__device__ __forceinline__ void sp_mfma_frags(f32x4 (&acc)[RB], const f32x4 (&a)[RB][4], const f32x4 (&b)[4], int d) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (16 * j < d) {
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][j][s], b[j][s], acc[rb], 0, 0, 0);
        }
    }
}

// any d: both operands re-read (L1 / L2) fragment by fragment
template <int RB>
__device__ __forceinline__ void sp_mfma_reread(f32x4 (&acc)[RB], const float* (&arow)[RB],const float* __restrict__ brow, int lg,
                                               int d, bool vec) {
    const int nkc = (d + 15) >> 4;
    for (int j = 0; j < nkc; ++j) {
        const f32x4 b = sp_load4(brow, 16 * j + 4 * lg, d, vec);
        f32x4 a[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) a[rb] = sp_load4(arow[rb], 16 * j + 4 * lg, d, vec);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) acc[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rb][s], b[s], acc[rb], 0, 0, 0);
    }
}

}  // namespace
