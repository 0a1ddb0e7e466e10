// dr_kn_kernel of gemm_dr.h -- the input gradient and the cached-W^T forward as split-K slabs, both operands straight into
// registers -- with its split count gd_dr_kn_splits and its entry point gd_dr_kn_launch.
#include <stdlib.h>

#include "gemm_dr.h"
#include "tail_job.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// C[M,N] = A[M,K] * B[K,N] as split-K partial slabs, A K-contiguous, B row-contiguous along N (the input gradient
// dh = dZ * W of reference main.py:350 / models/DNN.py:83-86: A = dZ [batch, items], B = the output layer's weight [items, hidden]).
// Round 4, end: both operands go STRAIGHT into the MFMA register layout -- no LDS at all, no barrier, no inline asm:
//   A as in dr_fat_kernel: lane (r, q) loads A[m0 + 16 a + r][k0 + 4 q .. + 3], component s feeds the MFMA whose k slot q stands
//     for k0 + 4 q + s;
//   B as in dr_tn_kernel: load (s, l) brings rows k0 + 4 q + s, columns n0 + 64 l + 4 r .. + 3; register e is the operand of the
//     block whose sixteen columns are n0 + 64 l + 4 r + e -- so a lane ends with four CONSECUTIVE columns (e) per row.
// One wave per SIMD owns an 80 x (64 NL) tile over one K range (5 x 4 NL accumulator blocks): per 16-deep chunk 80 NL MFMAs beside
// 5 + 4 NL loads (0.08 other instructions per MFMA; the LDS-tiled kernel that served this product: 0.35 and a barrier per 80,
// MFMA pipe busy 0.72).  Tasks (split, tile) are dealt statically, the tiles of one split to one XCD (they share its rows of B).
// The slabs go to the same reducer as before (gd_splitk_reduce: row scale, tanh').  Deterministic: static assignment, fixed k order.
// The passenger: a launch deals ntasks <= 4 gridDim.x tasks, and a workgroup whose four slots all lie past them exits at
// once -- its CU stands empty for the whole product.  With a tail job (job.on), the FIRST such workgroup in slot order runs the job
// (tail_job.h: row-partial reducer, float64 loss tail, row scale -- nothing the product reads) and exits; it hands over to nobody
// inside the launch, every other workgroup runs what it ran before.  The launch's dynamic LDS is the job's (none without one).
// ---------------------------------------------------------------------------------------------------------------------
#ifndef GD_KN_EVERY
#define GD_KN_EVERY 4
#endif
template <int NL>
__global__ __launch_bounds__(256, 1) void dr_kn_kernel(const DrArgs d, const GdTailJob job) {
    constexpr int TMB = 5;
    const GdGemm& g = d.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int nblk = gridDim.x, per = nblk >> 3;
    const int slot = (nblk & 7) == 0 ? ((int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3)) : (int)blockIdx.x;
    const int wl = slot * 4 + wave;
    const int n_waves = nblk * 4;
    const int ntiles = d.tiles_m * d.tiles_n;
    const int CPS = d.ksp;                      // chunks of 16 k per split (even)
    const int total_chunks = (g.K + 15) >> 4;
    const int ntasks = ntiles * g.splits;
    if (job.on && slot == (ntasks + 3) >> 2) {  // the first workgroup without a task: the passenger's
        extern __shared__ __attribute__((aligned(16))) unsigned char kn_lds[];
        gd_tail_job_run(job, kn_lds);
        return;
    }
    const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, (int)(((int64_t)(g.M - 1) * g.lda + g.K) * 4), 0x00020000);
    // (rows k >= K of B lie outside the descriptor and read as 0)
    const __amdgpu_buffer_rsrc_t srdB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, (int)(((int64_t)(g.K - 1) * g.ldb + g.N) * 4), 0x00020000);
    const uint32_t ldb16 = (uint32_t)g.ldb * 64u;  // bytes per chunk of 16 rows of B
    for (int task = wl; task < ntasks; task += n_waves) {
        const int split = task / ntiles, tile = task - split * ntiles;
        const int tm = tile % d.tiles_m, tn = tile / d.tiles_m;
        const int m0 = tm * (16 * TMB), n0 = tn * (64 * NL);
        const int c_lo = split * CPS;
        uint32_t offA[TMB], offB[4][NL];
#pragma unroll
        for (int a = 0; a < TMB; ++a) offA[a] = (uint32_t)(((int64_t)min(m0 + 16 * a + r, g.M - 1) * g.lda + 4 * q) * 4);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const int n = n0 + 64 * l + 4 * r;
                // a group that would start past the row's N columns is parked outside the matrix (reads 0)
                offB[s][l] = n < g.N ? (uint32_t)(((int64_t)(4 * q + s) * g.ldb + n) * 4) : 0x80000000u;
            }
        f32x4 acc[TMB][NL][4];
#pragma unroll
        for (int a = 0; a < TMB; ++a)
#pragma unroll
            for (int l = 0; l < NL; ++l)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[a][l][e] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 xa[2][TMB], xb[2][4][NL];
        {   // fill: chunk c_lo
            const uint32_t ka = (uint32_t)c_lo * 64u, kb = (uint32_t)c_lo * ldb16;
#pragma unroll
            for (int a = 0; a < TMB; ++a) xa[0][a] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, offA[a], ka, 0));
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int l = 0; l < NL; ++l)
                    xb[0][s][l] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdB, offB[s][l], kb, 0));
        }
        // one chunk: PAR = its parity; the 5 + 4 NL loads of chunk c + 1 ride between its first MFMAs, one every GD_KN_EVERY -- early, so
        // that the rest of the chunk covers their latency (B comes from HBM)
#define GD_KN_CHUNK(PAR, c)                                                                                            \
        {                                                                                                              \
            const bool more = (c) + 1 < c_lo + CPS && (c) + 1 < total_chunks;                                          \
            const uint32_t ka = more ? (uint32_t)((c) + 1) * 64u : 0x80000000u;                                        \
            const uint32_t kb = more ? (uint32_t)((c) + 1) * ldb16 : 0x80000000u;                                      \
            if ((c) * 16 + 15 >= g.K) { /* the chunk that reaches past K: zero A's k >= K (B's rows there read as 0) */ \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                        \
                    const bool keep = (c) * 16 + 4 * q + e < g.K;                                                      \
                    _Pragma("unroll") for (int a = 0; a < TMB; ++a) xa[PAR][a][e] = keep ? xa[PAR][a][e] : 0.f;        \
                }                                                                                                      \
            }                                                                                                          \
            /* (operands stay in VGPRs: hipcc otherwise parks them in spare AGPRs and moves them back per use) */        \
            _Pragma("unroll") for (int a = 0; a < TMB; ++a) asm volatile("" : "+v"(xa[PAR][a]));                       \
            _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                              \
                _Pragma("unroll") for (int l = 0; l < NL; ++l) asm volatile("" : "+v"(xb[PAR][s][l]));                 \
            __builtin_amdgcn_sched_barrier(0);                                                                         \
            _Pragma("unroll") for (int s = 0; s < 4; ++s) {                                                            \
                _Pragma("unroll") for (int n = 0; n < TMB * NL * 4; ++n) {                                             \
                    const int a = n / (NL * 4), l = (n / 4) % NL, e = n % 4;                                           \
                    acc[a][l][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[PAR][a][s], xb[PAR][s][l][e], acc[a][l][e], 0, 0, 0); \
                    const int idx = s * (TMB * NL * 4) + n;                                                            \
                    if (idx % GD_KN_EVERY == 2 && idx / GD_KN_EVERY < TMB + 4 * NL) {                                  \
                        const int ld = idx / GD_KN_EVERY;                                                              \
                        __builtin_amdgcn_sched_barrier(0);                                                             \
                        if (ld < TMB)                                                                                  \
                            xa[(PAR) ^ 1][ld] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, offA[ld], ka, 0)); \
                        else                                                                                           \
                            xb[(PAR) ^ 1][(ld - TMB) / NL][(ld - TMB) % NL] = __builtin_bit_cast(                      \
                                f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdB, offB[(ld - TMB) / NL][(ld - TMB) % NL], kb, 0)); \
                        __builtin_amdgcn_sched_barrier(0);                                                             \
                    }                                                                                                  \
                }                                                                                                      \
                __builtin_amdgcn_sched_barrier(0);                                                                     \
            }                                                                                                          \
        }
        for (int c = c_lo; c < c_lo + CPS && c < total_chunks; c += 2) {
            GD_KN_CHUNK(0, c);
            GD_KN_CHUNK(1, c + 1);
        }
#undef GD_KN_CHUNK
        // ---- epilogue: the partial tile into slab `split`; lane (r, q) owns columns n0 + 64 l + 4 r .. + 3 of rows 16 a + 4 q + t ----
        float* __restrict__ slab = g.C + (int64_t)split * g.slab_stride;
#pragma unroll
        for (int a = 0; a < TMB; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int m = m0 + 16 * a + 4 * q + t;
                if (m >= g.M) continue;
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    const int n = n0 + 64 * l + 4 * r;
                    const f32x4 v = {acc[a][l][0][t], acc[a][l][1][t], acc[a][l][2][t], acc[a][l][3][t]};
                    if (n + 3 < g.ldc) {  // (slab rows are round4(N) wide: a whole group or nothing)
                        *reinterpret_cast<f32x4*>(slab + (int64_t)m * g.ldc + n) = v;
                    } else {
                        for (int e = 0; e < 4; ++e)
                            if (n + e < g.N) slab[(int64_t)m * g.ldc + n + e] = v[e];
                    }
                }
            }
    }
}

}  // namespace

// dr_kn_kernel: 80 x 128 tiles, one (split, tile) task per wave slot (4 per CU): as many splits as fill the slots once -- or 0 when the
// product is not one the kernel takes (switched off, rows that do not tile by 80 within 12 %, a reduction too short to split, few slots).
int gd_dr_kn_splits(int M, int N, int K) {
    if (!dr_routes().kn || M < 16 || N < 64 || K < 4096) return 0;
    const long tiles = (long)gd_cdiv(M, 80) * gd_cdiv(N, 128);
    if ((long)gd_cdiv(M, 80) * 80 * 100 > (long)M * 112) return 0;  // 80-row tiles: at most 12 % padding
    if ((long)gd_cdiv(N, 128) * 128 * 100 > (long)N * 112) return 0;
    const long slots = 4L * dr_cu_count();
    if (tiles > slots) return 0;
    int splits = (int)(slots / tiles);
    const int total_chunks = gd_cdiv(K, 16);
    if (splits > total_chunks / 8) splits = total_chunks / 8;  // at least eight chunks per split
    if (splits < 2 || splits > 64) return splits > 64 ? 64 : 0;
    return splits;
}

// Whether a launch of dr_kn_kernel on n_cu workgroups over `ntasks` (split, tile) tasks leaves a workgroup without any: workgroup slot
// s owns tasks 4 s .. 4 s + 3 of the first round, so the first idle one is slot ceil(ntasks / 4).
static bool kn_idle_workgroup(int ntasks, int n_cu) { return gd_cdiv(ntasks, 4) < n_cu; }

#ifndef GD_KN_TAIL_DEFAULT
#define GD_KN_TAIL_DEFAULT 1  // GDMCF_KN_TAIL when the environment does not set it
#endif

// The input gradient as split-K slabs on dr_kn_kernel (sets g.splits / kchunk / tiles_* for the reducer), or GD_DR_NOT_TAKEN with g
// as it was.  job (may be NULL): a tail job that must ride the launch -- declined with GD_DR_NOT_TAKEN where it cannot.
static int kn_launch(GdGemm& g, const GdTailJob* job, hipStream_t s) {
    if (!dr_routes().kn) return GD_DR_NOT_TAKEN;
    const int splits = gd_dr_kn_splits(g.M, g.N, g.K);
    const size_t need = (size_t)splits * g.M * g.ldc * sizeof(float);
    const bool ok = splits > 0 && g.ldc >= g.N && (g.ldc & 3) == 0 && g.ws_cap >= need && g.slab_stride >= (int64_t)g.M * g.ldc &&
                (int64_t)g.M * g.lda * 4 < ((int64_t)1 << 31) && (int64_t)g.K * g.ldb * 4 < ((int64_t)1 << 31) && g.lda >= g.K && g.ldb >= g.N &&
                (reinterpret_cast<uintptr_t>(g.B) & 15) == 0 && (g.ldb & 3) == 0 && (reinterpret_cast<uintptr_t>(g.C) & 15) == 0;
    if (!ok) return GD_DR_NOT_TAKEN;
    DrArgs d = {};
    const int n_cu = dr_cu_count();
    const int total_chunks = gd_cdiv(g.K, 16);
    const int cps = (gd_cdiv(total_chunks, splits) + 1) & ~1;  // chunks per split, even (the loop runs them in pairs)
    const int real_splits = gd_cdiv(total_chunks, cps);
    d.tiles_m = gd_cdiv(g.M, 80);
    d.tiles_n = gd_cdiv(g.N, 128);
    d.ksp = cps;
    GdTailJob none = {};
    size_t lds = 0;
    if (job) {
        const bool tail_on = gd_env_int("GDMCF_KN_TAIL", GD_KN_TAIL_DEFAULT) != 0;  // (read at every call: one process can time and test both)
        lds = lt_lds_bytes(job->T, job->H, job->B);
        if (!tail_on || !job->on || !kn_idle_workgroup(d.tiles_m * d.tiles_n * real_splits, n_cu) || lds > GD_LT_LDS_MAX)
            return GD_DR_NOT_TAKEN;
        static bool attr_set = false;
        if (!gd_allow_big_lds(dr_kn_kernel<2>, lds, &attr_set, "gemm_dr_kn")) return GDMCF_E_HIP;
    }
    g.splits = real_splits;
    g.kchunk = cps * 16;
    g.tiles_m = d.tiles_m;
    g.tiles_n = d.tiles_n;
    d.g = g;
    {
        GdProfScope prof(g.prof_tag, 2.0 * g.M * g.N * g.K, s);
        hipLaunchKernelGGL((dr_kn_kernel<2>), dim3(n_cu), dim3(256), lds, s, d, job ? *job : none);
    }
    t_gd_last_gemm = 5;
    return gd_launch_status("gemm_dr_kn");
}

int gd_dr_kn_launch(GdGemm& g, hipStream_t s) { return kn_launch(g, nullptr, s); }
int gd_dr_kn_launch_tail(GdGemm& g, const GdTailJob& job, hipStream_t s) { return kn_launch(g, &job, s); }

int gdmcf_debug_kn_tail_rides(int M, int N, int K) {
    const int splits = gd_dr_kn_splits(M, N, K);
    if (splits <= 0) return 0;
    const int total_chunks = gd_cdiv(K, 16);
    const int cps = (gd_cdiv(total_chunks, splits) + 1) & ~1;
    return kn_idle_workgroup(gd_cdiv(M, 80) * gd_cdiv(N, 128) * gd_cdiv(total_chunks, cps), dr_cu_count()) ? 1 : 0;
}
