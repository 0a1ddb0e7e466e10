// "Direct-to-register" f32 MFMA products: no LDS, no barriers, independent persistent waves.
//
// v_mfma_f32_16x16x4_f32 runs at 1/16 of the bf16 matrix rate, so an operand byte is worth sixteen times more matrix
// time than in a bf16 kernel: a wave can afford to fetch its OWN operands from L1/L2 straight into the MFMA register
// layout.  What that buys (measured, tools/dr_probe.hip): no LDS round trip, no workgroup barrier -- hence
// no lockstep between waves, a wave that waits for memory or stores its results leaves the matrix pipe to its SIMD
// partner -- output tiles small enough (64 x 64 per wave) to balance 8 600 of them over 1 024 SIMDs from a ticket counter,
// and results that leave the accumulators as 16 contiguous bytes per lane.
//
// The kernels (gdmcf_debug_last_gemm family code in brackets), one file per pipeline, each behind a route switch of DrRoutes, all
// on by default; a product a kernel does not take, or whose switch is off, goes to the LDS-tiled kernels (gemm_f32.hip):
//   gemm_dr_tn.hip   dr_tn_kernel        [2]  weight gradient dW = dZ^T A: ring of registers, asm loads, ticket queues    GDMCF_DR_DW
//                    dr_tn_adamw_kernel  [3]  the same with the AdamW update in the epilogue, up to four products per launch  GDMCF_DR_DW, _ADAMW
//   gemm_dr_fat.hip  dr_fat_kernel       [4]  the output layer with a fused row-loss / posterior epilogue                 GDMCF_DR_FAT
//                                        [6]  the same loop over a K range per task: the first-layer forward as split-K slabs  GDMCF_DR_FAT_SLAB
//   gemm_dr_kn.hip   dr_kn_kernel        [5]  the input gradient and the cached-W^T forward as split-K slabs               GDMCF_DR_KN
//   gemm_dr.hip      the switches, the CU count and gd_gemm_dr_launch: the common refusals and the (layA, layB, epi) dispatch
// Who calls: gd_gemm_launch (gemm_f32.hip) offers every f32 product to gd_gemm_dr_launch ahead of the LDS-tiled families; linear.hip
// calls gd_gemm_dr_adamw_multi for its list entry and gd_dr_kn_launch_tail (tail_job.h) for the input gradient that carries a tail job.
//
// Each kernel file exports ONE take-or-decline function (below).  It owns everything that belongs to its kernel -- the route
// switch, the shape / alignment / 32-bit-offset predicates, the GdProfScope, the family code, the launch -- and either launches
// or returns GD_DR_NOT_TAKEN with the caller's GdGemm exactly as it found it.
#pragma once

#include "common.h"

// (in an anonymous namespace, as the kernels that take it by value are in each file: their symbols name the type)
namespace {
struct DrArgs {
    GdGemm g;
    int tiles_m, tiles_n, m_fastest;
    int ksp;      // k-steps run per tile (a multiple of the ring size; steps past K load zeros)
    int ctr;      // index into g_dr_ticket (dr_ticket_slot: a set of its own for every launch that may be in flight)
    const GdAdamHyper* adam_dev;  // fused AdamW: this step's scalars in device memory (graph replay), NULL = GdGemm::adam
    int stagger;  // waves 4-7 of a workgroup start this many x 3.4 us later (dr_tn_kernel); dr_fat_kernel reads it as its x_t
                  // prefetch distance, in chunks before the end of the k loop (GDMCF_FAT_PF)
};
}  // namespace

// Route switches: which products the kernels take (a product whose switch is off goes to the LDS-tiled kernels).  Read once, each
// variable on unless set to 0 (DESIGN.md lists them); one instance for the library (gemm_dr.hip); tools/gemm_probe.hip assigns to
// the struct directly.
struct DrRoutes {
    bool dw;     // GDMCF_DR_DW: f32 weight gradients, plain and fused-AdamW (dr_tn_kernel, dr_tn_adamw_kernel)
    bool adamw;  // GDMCF_DR_ADAMW: the fused-AdamW ones among them (dr_tn_adamw_kernel)
    bool kn;     // GDMCF_DR_KN: the input gradient and the cached-W^T forward (dr_kn_kernel; also sizes the workspace)
    bool fat;    // GDMCF_DR_FAT: the output layer with the fused row-loss / posterior epilogue (dr_fat_kernel)
    bool fat_slab;  // GDMCF_DR_FAT_SLAB: the first-layer forward as split-K slabs on dr_fat_kernel's LDS-DMA loop (also sizes the workspace)
};
DrRoutes& dr_routes();
int dr_cu_count();  // compute units of the current device
int dr_stagger();   // GDMCF_DR_STAGGER (dr_tn_kernel, dr_tn_adamw_kernel)

// take-or-decline, one per kernel file (the fused-AdamW products: gd_gemm_dr_adamw_multi, common.h)
int gd_dr_tn_launch(GdGemm& g, hipStream_t s);            // gemm_dr_tn.hip: layouts MC / MC, GD_EPI_STORE
int gd_dr_kn_launch(GdGemm& g, hipStream_t s);            // gemm_dr_kn.hip: layouts KC / MC, GD_EPI_SLAB
int gd_dr_fat_launch(int epi, GdGemm& g, hipStream_t s);  // gemm_dr_fat.hip: layouts KC / KC, GD_EPI_LOSS or GD_EPI_POST
int gd_dr_fat_slab_launch(GdGemm& g, hipStream_t s);      // gemm_dr_fat.hip: layouts KC / KC, GD_EPI_SLAB
