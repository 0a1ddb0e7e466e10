// What the dense product families share on the host (gemm_f32.hip, gemm_bf16.hip, gemm_split.hip, gemm_small.hip):
//   gd_gemm_variant   the (layA, layB, epi) variants a dense product comes in, mapped onto a family's launcher -- the only such switch
//   gd_tiled_launch   the launch of one LDS-tiled kernel over an [M, N] grid of tiles times the K splits
//   gd_allow_big_lds  the dynamic-LDS limit of a kernel that needs more than the default
// Host code only: a family keeps its kernels, its tile classes and whatever it checks or sets ahead of the dispatch.
#pragma once

#include "common.h"

namespace {

// raises `kernel`'s dynamic-LDS limit to `limit` bytes when `lds` needs more than the default 48 KiB, once per kernel (*done: the
// caller's static flag).  T = 1000 diffusion steps x 10 history entries need 88 KB.
template <class K>
bool gd_allow_big_lds(K* kernel, size_t lds, bool* done, const char* who, size_t limit = 160 * 1024) {
    if (*done || lds <= 48 * 1024) return true;
    *done = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) == hipSuccess;
    if (!*done) gdmcf_set_error("%s: hipFuncSetAttribute failed", who);
    return *done;
}

// The seven variants of a dense product: KC/KC x {SLAB, BIAS_ACT, LOSS, POST} (forward layers), KC/MC x SLAB (input gradient,
// cached-W^T forward), MC/MC x {STORE, ADAMW} (weight gradient).  Calls launch.operator()<LAYA, LAYB, EPI>(args...) for the one that
// (layA, layB, epi) names; anything else is GDMCF_E_UNSUPPORTED with the family's word ("", "bf16 ", ...) in the message.
template <class L, class... Args>
int gd_gemm_variant(const char* family, int layA, int layB, int epi, const L& launch, Args&&... args) {
#define GD_VARIANT(LA, LB, EPI) \
    if (layA == LA && layB == LB && epi == EPI) return launch.template operator()<LA, LB, EPI>(args...)
    GD_VARIANT(GD_LAY_KC, GD_LAY_KC, GD_EPI_SLAB);
    GD_VARIANT(GD_LAY_KC, GD_LAY_KC, GD_EPI_BIAS_ACT);
    GD_VARIANT(GD_LAY_KC, GD_LAY_KC, GD_EPI_LOSS);
    GD_VARIANT(GD_LAY_KC, GD_LAY_KC, GD_EPI_POST);
    GD_VARIANT(GD_LAY_KC, GD_LAY_MC, GD_EPI_SLAB);
    GD_VARIANT(GD_LAY_MC, GD_LAY_MC, GD_EPI_STORE);
    GD_VARIANT(GD_LAY_MC, GD_LAY_MC, GD_EPI_ADAMW);
#undef GD_VARIANT
    gdmcf_set_error("unsupported %sgemm variant (layA=%d layB=%d epi=%d)", family, layA, layB, epi);
    return GDMCF_E_UNSUPPORTED;
}

// One LDS-tiled kernel (BM x BN tiles, k steps of BK, `block` threads, `lds` bytes of dynamic LDS) over g: fills in g.tiles_m /
// tiles_n and the defaults of g.splits / kchunk, launches tiles_m * tiles_n * splits workgroups.  attr_done: the static flag of the
// caller's kernel; lds_limit: the dynamic-LDS limit that kernel asks for when it needs more than the default.
template <class K>
int gd_tiled_launch(K* kern, unsigned block, size_t lds, size_t lds_limit, int BM, int BN, int BK, bool* attr_done, const char* name,
                    GdGemm& g, hipStream_t s) {
    if (!gd_allow_big_lds(kern, lds, attr_done, name, lds_limit)) return GDMCF_E_HIP;
    g.tiles_m = gd_cdiv(g.M, BM);
    g.tiles_n = gd_cdiv(g.N, BN);
    if (g.splits < 1) g.splits = 1;
    if (g.kchunk <= 0) g.kchunk = gd_cdiv(gd_cdiv(g.K, g.splits), BK) * BK;
    const long grid = (long)g.tiles_m * g.tiles_n * g.splits;
    if (grid <= 0 || grid > 0x7fffffffL) {
        gdmcf_set_error("gemm grid out of range: %ld", grid);
        return GDMCF_E_SHAPE;
    }
    {
        GdProfScope prof(g.prof_tag, 2.0 * g.M * g.N * g.K, s);
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(block), lds, s, g);
    }
    return gd_launch_status(name);
}

}  // namespace
