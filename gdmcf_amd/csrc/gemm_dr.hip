// What the direct-to-register kernels of gemm_dr.h share on the host -- the route switches, the CU count, the stagger knob -- and
// gd_gemm_dr_launch: the refusals common to all of them, then the (layA, layB, epi) switch onto each kernel's take-or-decline.
#include <stdlib.h>

#include "gemm_dr.h"

int dr_cu_count() {
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 256;
    }
    return n_cu;
}

#ifndef GD_FAT_SLAB_DEFAULT
#define GD_FAT_SLAB_DEFAULT 1  // GDMCF_DR_FAT_SLAB when the environment does not set it
#endif

static bool dr_env_on(const char* name, bool dflt = true) { return gd_env_int(name, dflt) != 0; }
DrRoutes& dr_routes() {
    static DrRoutes r = {dr_env_on("GDMCF_DR_DW"), dr_env_on("GDMCF_DR_ADAMW"), dr_env_on("GDMCF_DR_KN"), dr_env_on("GDMCF_DR_FAT"),
                         dr_env_on("GDMCF_DR_FAT_SLAB", GD_FAT_SLAB_DEFAULT != 0)};
    return r;
}

int dr_stagger() {
    static const int stagger = gd_env_int("GDMCF_DR_STAGGER", 3);
    return stagger;
}

// Returns GD_DR_NOT_TAKEN when the product is not one these kernels handle (the caller falls back to the LDS-tiled kernels).
int gd_gemm_dr_launch(int layA, int layB, int epi, GdGemm& g, hipStream_t s) {
    if (g.bf16) return GD_DR_NOT_TAKEN;
    if (g.accumulate || g.C16 || (g.splits > 1 && epi != GD_EPI_SLAB)) return GD_DR_NOT_TAKEN;  // (slabs: the kernels set their own split count)
    if (layA == GD_LAY_MC && layB == GD_LAY_MC) {
        if (epi == GD_EPI_ADAMW) return gd_gemm_dr_adamw_multi(&g, 1, s);  // the one-element case
        if (epi == GD_EPI_STORE) return gd_dr_tn_launch(g, s);
    } else if (layA == GD_LAY_KC && layB == GD_LAY_MC) {
        if (epi == GD_EPI_SLAB) return gd_dr_kn_launch(g, s);
    } else if (layA == GD_LAY_KC && layB == GD_LAY_KC) {
        if (epi == GD_EPI_LOSS || epi == GD_EPI_POST) return gd_dr_fat_launch(epi, g, s);
        if (epi == GD_EPI_SLAB) return gd_dr_fat_slab_launch(g, s);
    }
    return GD_DR_NOT_TAKEN;
}
