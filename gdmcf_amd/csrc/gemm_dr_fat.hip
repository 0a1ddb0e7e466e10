// dr_fat_kernel of gemm_dr.h -- the output layer with a fused row-loss / posterior epilogue as one fat tile per wave, and the same loop
// over a K range per task for the first-layer forward as split-K slabs -- with its launcher and its entry points gd_dr_fat_launch and
// gd_dr_fat_slab_launch (plan: gd_dr_fat_slab_plan).
#include <stdlib.h>

#include "gemm_dr.h"

#ifndef GD_FAT_DMA_DEFAULT
#define GD_FAT_DMA_DEFAULT 1  // GDMCF_FAT_DMA when the environment does not set it
#endif

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// C[M,N] = A[M,K] * B[N,K]^T for a batch-sized A and a LARGE B with a fused row-loss / posterior epilogue (the output layer:
// reference models/DNN.py:83-86 with gaussian_diffusion.py:335 in training, :451-498 in the reverse loop), round 4:
// ONE FAT TILE PER WAVE, ONE WAVE PER SIMD, ONE PASS.
//
// What rounds 2-3 established about this product: the LDS-tiled kernel and the retired hybrid kernel both end at 0.6 of
// the matrix rate because (i) 1 345 / 2 690 tiles on 512 / 1 024 slots are 2.63 rounds -- a third of the chip runs three -- and
// (ii) the loop is bound by instruction ISSUE: v_mfma_f32_16x16x4_f32 shares the vector issue port, so every load, LDS access
// and barrier beside the MFMAs is matrix time lost (round 4: even another wave's arithmetic does not overlap).  Both have one
// cure: MORE OUTPUT PER WAVE.  A wave alone on its SIMD may use all 512 registers: 5 x NB accumulator blocks of 16 x 16 (NB =
// 11: 220 registers) hold an 80 x 176 tile, so the WHOLE [400 x 34 395] output is 980 tiles -- one per wave, 96 % of the 1 024
// SIMDs busy for the whole launch, no second round, no tail -- and per 16-deep k chunk the wave issues 220 MFMAs beside 16 loads,
// 11 LDS writes and 11 LDS reads (0.17 other instructions per MFMA; the LDS-tiled kernel: 0.35, plus a barrier per 80).
//   * A (the hidden activations, L2-resident) is loaded straight into the MFMA layout: lane (j = lane & 15, q = lane >> 4) reads
//     A[m0 + 16 i + j][k0 + 4 q .. + 3] -- one 16-byte load per row block and chunk; component s is the operand of the MFMA that
//     takes k = k0 + 4 q + s (A and B permuted alike).  1.6 MB read by every wave: half lines are no concern here (they were for
//     the STREAMED operand of the retired K-contiguous register-streaming kernel).
//   * B (the weight, streamed from HBM once per row tile: the five row tiles of a column panel run on one XCD) is fetched in
//     pieces of 16 rows x 64 B, staged in registers for two k steps, written to a wave-PRIVATE LDS image (rows of 16 floats,
//     16-byte slot s of row r at s ^ 2 ((r >> 2) & 1): conflict-free for the ds_read_b128 lane groups) and read back as
//     fragments -- ordered by the wave's own LDS queue, no barrier.
//   * No instruction of the loop is inline asm: every load of a chunk is waited for inside the chunk that issued it (nothing is
//     in flight across the loop's back edge), so hipcc's own counted waits are exact; sched_barriers pin the placement.
// acc[i][b][t] = C[m0 + 16 i + 4 q + t][n0 + 16 b + r].  Deterministic: fixed k order, one wave per tile, static assignment.
//
// DMA = 1 (GDMCF_FAT_DMA): the same loop with B's pieces loaded STRAIGHT INTO THE LDS IMAGE by LDS-DMA (buffer_load_dwordx4
// ... lds, 16 bytes per lane) -- no staging registers G, no ds_write_b128: 11 of a chunk's 38 non-MFMA instructions less (NB = 11).
// Same MFMAs, same operands, same k order: bit-identical to DMA = 0, which stays as the route for sources that are not 16-byte
// aligned and as the A/B partner.
//   * An LDS-DMA load writes wave-uniform base + lane x 16 B: lane l of piece p lands at row l >> 2, PHYSICAL slot l & 3.  The image
//     keeps its conflict-free swizzle (what r_off reads is unchanged), so the swizzle moves to the SOURCE: lane l fetches the
//     global slot (l & 3) ^ 2 ((row >> 2) & 1) of its row, the one whose place in the image is l & 3.
//   * hipcc puts NO wait between an LDS-DMA load and a ds_read of the bytes it writes, and the hardware orders the two by
//     nothing but the issuing wave's vmcnt.  Every chunk therefore opens with s_waitcnt vmcnt(0) between sched_barriers, before
//     its first fragment read: that retires the pieces the previous chunk (or the fill) issued into this chunk's image, and with
//     them A's loads and the posterior's x_t touches -- nothing is in flight across a chunk boundary, no count is needed.
//     The build disassembles this file and fails if any ds_read_b128 follows a ... lds load without such a wait (build.py).
//   * WAR: the pieces of chunk c + 1 go into the image that chunk c - 1 read; those fragments were MFMA operands of chunk c - 1,
//     so their ds_reads have retired.  The last chunk's parked loads (range-checked: no fetch, zeros) still WRITE their image:
//     a vmcnt(0) after the loop retires them before the epilogue stages rows in the same LDS, and the fill of the NEXT tile waits
//     lgkmcnt(0) for the epilogue's last reads of that staging.
//
// EPI = GD_EPI_SLAB (GDMCF_DR_FAT_SLAB): the first-layer forward xin W1^T, a [batch x hidden] output over a LONG K.  A task is
// (split, tile): the same chunk bodies over the chunks [c_lo, c_hi) of one split, the partial tile stored into slab `split` for
// gd_splitk_reduce.  Everything slab-specific is behind `SLAB` and folds to the fused epilogues' constants otherwise.
// ---------------------------------------------------------------------------------------------------------------------
template <int NB, int EPI, int DMA>
__global__ __launch_bounds__(256, 1) void dr_fat_kernel(const DrArgs d) {
    static_assert(EPI == GD_EPI_LOSS || EPI == GD_EPI_POST || EPI == GD_EPI_SLAB, "output layer with a fused epilogue, or split-K slabs");
    static_assert(NB >= 4 && NB <= 12, "5 x NB accumulator blocks must fit 256 registers");
    static_assert(DMA == 0 || DMA == 1, "B through staging registers, or straight into LDS");
    constexpr bool SLAB = EPI == GD_EPI_SLAB;
    typedef __attribute__((address_space(3))) void* lds_vp;
    constexpr int WAIT_VM0 = 0x0F70, WAIT_LGKM0 = 0xC07F;  // s_waitcnt vmcnt(0) / lgkmcnt(0), the other counters left alone
    constexpr int TMB = 5;
    const GdGemm& g = d.g;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    extern __shared__ __attribute__((aligned(16))) float dr_lds[];
    float* const lds = dr_lds + wave * (2 * NB * 256);  // two chunk images of 16 NB rows x 16 floats
    // consecutive tiles (the row tiles of one column panel first) on consecutive waves of ONE XCD: blocks b and b + 8 share an XCD
    const int nblk = gridDim.x, per = nblk >> 3;
    const int wl = ((nblk & 7) == 0 ? ((int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3)) : (int)blockIdx.x) * 4 + wave;
    const int n_waves = nblk * 4;
    const int ntiles = d.tiles_m * d.tiles_n;
    const __amdgpu_buffer_rsrc_t srdA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A), 0, (int)(((int64_t)(g.M - 1) * g.lda + g.K) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t srdB = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.B), 0, (int)(((int64_t)(g.N - 1) * g.ldb + g.K) * 4), 0x00020000);
    const int NCH = d.ksp;       // chunks of 16 k per tile: ceil(K / 16) -- the loop runs them in pairs, an odd last one alone
    const int c_mask = g.K >> 4;  // first chunk that reaches past K
    const int ntasks = SLAB ? ntiles * g.splits : ntiles;  // slabs: a task is (split, tile), the tiles of one split on consecutive waves
    // LDS float offsets: write -- piece p = rows 16 p + (lane >> 2), slot lane & 3; read -- block b = rows 16 b + r, slot q
    // (DMA: the write lands lane-linear, row lane >> 2, slot lane & 3; the lane fetches the global slot g_slot that belongs there)
    const int w_off = (lane >> 2) * 16 + (((lane & 3) ^ ((((lane >> 2) >> 2) & 1) << 1)) << 2);
    const int g_slot = DMA ? ((lane & 3) ^ ((((lane >> 2) >> 2) & 1) << 1)) : (lane & 3);
    const int r_off = r * 16 + ((q ^ (((r >> 2) & 1) << 1)) << 2);
    for (int task = wl; task < ntasks; task += n_waves) {
        // slabs: this task's chunks [c_lo, c_hi) of the reduction, the whole ones [c_lo, c_in); a chunk that reaches past K is the
        // last split's last (c_hi > c_in).  The fused epilogues: one tile per task, every chunk.
        const int split = SLAB ? task / ntiles : 0;
        const int tile = SLAB ? task - split * ntiles : task;
        const int c_lo = SLAB ? split * (g.kchunk >> 4) : 0;
        const int c_hi = SLAB ? min(c_lo + (g.kchunk >> 4), NCH) : NCH;
        const int c_in = SLAB ? min(c_hi, c_mask) : c_mask;
        const int tm = tile % d.tiles_m, tn = tile / d.tiles_m;
        const int m0 = tm * (16 * TMB), n0 = tn * (16 * NB);
        uint32_t offA[TMB], offB[NB];
#pragma unroll
        for (int i = 0; i < TMB; ++i) offA[i] = (uint32_t)((m0 + 16 * i + r) * g.lda + 4 * q) * 4u;
#pragma unroll
        for (int p = 0; p < NB; ++p) offB[p] = (uint32_t)(((int64_t)(n0 + 16 * p + (lane >> 2)) * g.ldb + 4 * g_slot) * 4);
        f32x4 acc[TMB][NB];
#pragma unroll
        for (int i = 0; i < TMB; ++i)
#pragma unroll
            for (int b = 0; b < NB; ++b) acc[i][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 xa[2][TMB], G[DMA ? 1 : NB], FB[NB];
        // ---- fill: chunk 0 of A into xa[0], chunk 0 of B through LDS image 0 (DMA: into the registers and the image of parity hp,
        // see the loop) ----
        const int hp = DMA ? ((c_in - c_lo) & 1) : 0;  // (slabs: the parity of this task's whole-chunk count)
        const int k_lo = SLAB ? c_lo * 64 : 0;         // scalar byte offset of the task's first chunk
        if (hp) {
#pragma unroll
            for (int i = 0; i < TMB; ++i) xa[1][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, offA[i], k_lo, 0));
        } else {
#pragma unroll
            for (int i = 0; i < TMB; ++i) xa[0][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdA, offA[i], k_lo, 0));
        }
        if constexpr (DMA) {
            // (the previous tile's epilogue has read its row staging out of this LDS: those reads retire before a piece may land)
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(WAIT_LGKM0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p = 0; p < NB; ++p) __builtin_amdgcn_raw_ptr_buffer_load_lds(srdB, (lds_vp)(lds + hp * (NB * 256) + p * 256), 16, (int)offB[p], k_lo, 0, 0);
        } else {
#pragma unroll
            for (int p = 0; p < NB; ++p) G[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srdB, offB[p], k_lo, 0));
#pragma unroll
            for (int p = 0; p < NB; ++p) *reinterpret_cast<f32x4*>(lds + p * 256 + w_off) = G[p];
        }

        // one chunk: PAR = its parity (A registers xa[PAR], LDS image PAR); the loads of chunk c + 1 ride in k steps 0 and 1,
        // its LDS writes in k step 3 (DMA: the pieces go straight into the other image, and the chunk opens with the wait that
        // retires everything the previous chunk issued -- the pieces of ITS image first of all -- before the first fragment read)
#define GD_FAT_CHUNK(PAR, c, MSK)                                                                                         \
        {                                                                                                             \
            /* scalar offset of the next chunk; past the task's last chunk it parks the loads outside both matrices (0, no fetch) */ \
            const uint32_t kn = ((c) + 1 < c_hi) ? (uint32_t)((c) + 1) * 64u : 0x80000000u;                           \
            if constexpr (DMA) {                                                                                      \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
                __builtin_amdgcn_s_waitcnt(WAIT_VM0);                                                                 \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
            }                                                                                                         \
            _Pragma("unroll") for (int b = 0; b < NB; ++b)                                                            \
                FB[b] = *reinterpret_cast<const f32x4*>(lds + (PAR) * (NB * 256) + b * 256 + r_off);                  \
            if (MSK) { /* the chunk(s) that reach past K: zero every k >= K of both operands (what lies behind a row's K */ \
                /* elements -- the next row, or the padding of a leading dimension > K -- may hold anything, NaN included) */ \
                _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                       \
                    const bool keep = (c) * 16 + 4 * q + e < g.K;                                                     \
                    _Pragma("unroll") for (int i = 0; i < TMB; ++i) xa[PAR][i][e] = keep ? xa[PAR][i][e] : 0.f;       \
                    _Pragma("unroll") for (int b = 0; b < NB; ++b) FB[b][e] = keep ? FB[b][e] : 0.f;                  \
                }                                                                                                     \
            }                                                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
            _Pragma("unroll") for (int sx = 0; sx < 4; ++sx) {                                                        \
                _Pragma("unroll") for (int n = 0; n < TMB * NB; ++n) {                                                \
                    const int i = n / NB, b = n % NB;                                                                 \
                    if (sx == 0 && i == 0) asm volatile("" : "+v"(FB[b])); /* (operands stay in VGPRs: hipcc otherwise parks them in spare AGPRs) */ \
                    if (sx == 0 && b == 0) asm volatile("" : "+v"(xa[PAR][i]));                                       \
                    acc[i][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[PAR][i][sx], FB[b][sx], acc[i][b], 0, 0, 0);  \
                    /* loads of the next chunk: A's five and the first pieces of B in k step 0, the rest in k step 1 */ \
                    if (sx < 2 && n % 5 == 2) { /* k step 0 carries loads 0 .. NB - 1, k step 1 the remaining TMB */     \
                        const int l = (sx == 0) ? n / 5 : NB + n / 5;                                                 \
                        if (l < TMB + NB) {                                                                           \
                            __builtin_amdgcn_sched_barrier(0);                                                        \
                            if (l < TMB)                                                                              \
                                xa[(PAR) ^ 1][l] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(   \
                                    srdA, offA[l], kn, 0));                                                           \
                            else if constexpr (DMA)                                                                   \
                                __builtin_amdgcn_raw_ptr_buffer_load_lds(                                             \
                                    srdB, (lds_vp)(lds + ((PAR) ^ 1) * (NB * 256) + (l - TMB) * 256), 16,             \
                                    (int)offB[l - TMB], (int)kn, 0, 0);                                               \
                            else                                                                                      \
                                G[l - TMB] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(         \
                                    srdB, offB[l - TMB], kn, 0));                                                     \
                            __builtin_amdgcn_sched_barrier(0);                                                        \
                        }                                                                                             \
                    }                                                                                                 \
                    if (!DMA && sx == 3 && n % 4 == 1 && n / 4 < NB) { /* the pieces have landed: into the other LDS image */ \
                        __builtin_amdgcn_sched_barrier(0);                                                            \
                        *reinterpret_cast<f32x4*>(lds + ((PAR) ^ 1) * (NB * 256) + (n / 4) * 256 + w_off) = G[n / 4]; \
                        __builtin_amdgcn_sched_barrier(0);                                                            \
                    }                                                                                                 \
                }                                                                                                     \
                __builtin_amdgcn_sched_barrier(0);                                                                    \
            }                                                                                                         \
        }
        // Reverse step: the epilogue reads the tile's x_t (80 x 16 NB floats per wave, 55 MB per launch at the Yelp shape) in the same
        // burst in which every wave writes x_{t-1} -- the only HBM-bound stretch of the kernel, while the k loop leaves HBM nearly
        // idle.  Some chunks (default ten, ~30 us) before the end the wave touches one dword of every 128-byte line of its x_t tile with LDS-DMA
        // loads (buffer_load_dword ... lds into a scratch line of its own: no registers; DMA = 0: nothing waits for them, DMA = 1: they
        // retire with everything else at the next chunk's opening vmcnt(0), some 7 000 cycles of MFMAs later), so the epilogue's
        // reads find the lines in L2 / the Infinity Cache.
        const int c_pf = d.stagger > 0 ? ((NCH > d.stagger + 2 ? NCH - d.stagger : 0) & ~1) : -2;  // (d.stagger: chunks before the end; 0 = off)
        // DMA = 0 asks every chunk whether it reaches past K; the two arms of that branch meet in 32 register copies per chunk.
        // DMA = 1 does not ask.  At most ONE chunk reaches past K, the last (NCH - c_mask <= 1): it is an instantiation of its own,
        // at parity 0, behind a pair loop that runs only chunks inside K.  The parities are labels (which registers, which image),
        // so an odd number of inside chunks is evened out in FRONT: chunk 0 then runs alone at parity 1, which is where the fill put
        // it (hp).  Same chunks, same k order, same MFMAs as DMA = 0.
        // Slabs: the same four bodies over the task's range [c_lo, c_hi) -- chunk c_lo alone at parity 1 when the count of whole chunks
        // is odd, the pairs up to c_in, then the masked chunk if this task has it (the last split only; it may be the task's only chunk:
        // hp is then 0 and the fill has put it at parity 0, where the masked body reads).
        const int c_pairs = DMA ? c_in : c_hi;                                            // the pair loop runs chunks [c_lo + hp, c_pairs)
        const int c_pfl = (DMA && c_pf >= 0) ? min(c_pf | hp, c_pairs - 2) : c_pf;         // (the touches ride on a pair of the loop)
        int c = c_lo;
        if constexpr (DMA) {
            if (hp) {
                GD_FAT_CHUNK(1, c_lo, false);
                c = c_lo + 1;
            }
        }
        for (; c + 1 < c_pairs; c += 2) {
            if constexpr (EPI == GD_EPI_POST) {
                if (c == c_pfl) {
                    constexpr int NJL = (16 * NB * 4 + 127) / 128 + 1;   // touches per row: one per line + the row's last element
                    constexpr int NPI = (80 * NJL + 63) / 64;
                    float* const scratch = dr_lds + 4 * (2 * NB * 256) + wave * 64;
                    const __amdgpu_buffer_rsrc_t srdX = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<float*>(g.aux), 0, (int)(((int64_t)(g.M - 1) * g.ldaux + g.N) * 4), 0x00020000);
#pragma unroll
                    for (int pi = 0; pi < NPI; ++pi) {
                        const int t = min(pi * 64 + lane, 80 * NJL - 1);
                        const int row = min(m0 + t % 80, g.M - 1), j = t / 80;
                        const int col = min(j < NJL - 1 ? n0 + 32 * j : n0 + 16 * NB - 1, g.N - 1);
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(srdX, (lds_vp)scratch, 4, (int)(((int64_t)row * g.ldaux + col) * 4), 0, 0, 0);
                    }
                }
            }
            if constexpr (DMA) {
                GD_FAT_CHUNK(0, c, false);
                GD_FAT_CHUNK(1, c + 1, false);
            } else {
                GD_FAT_CHUNK(0, c, c >= c_mask);
                GD_FAT_CHUNK(1, c + 1, c + 1 >= c_mask);
            }
        }
        // an odd number of chunks (K = 1 000: 63, the last one half masked): the last chunk alone, not a pair with an all-zero
        // partner (1.6 % of the product's matrix instructions at K = 1 000)
        if constexpr (DMA) {
            if (c < c_hi) GD_FAT_CHUNK(0, c, true);  // (c == c_mask here)
        } else {
            if ((c_hi - c_lo) & 1) GD_FAT_CHUNK(0, c_hi - 1, c_hi - 1 >= c_mask);
        }
#undef GD_FAT_CHUNK
        if constexpr (DMA) {
            // the last chunk's parked pieces write zeros into the image the epilogue is about to stage rows in: retired first
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(WAIT_VM0);
            __builtin_amdgcn_sched_barrier(0);
        }

        if constexpr (SLAB) {
            // ---- slab epilogue: the partial tile into slab `split`, staged in rows as below -- no bias, no global reads.  The slab's
            // rows are ldc = round4(N) floats and 16-byte aligned: whole groups leave as 16-byte stores, the group that holds column
            // N - 1 element by element (a store past N would land in the next row), rows >= M not at all ----
            constexpr int LDS_S = 16 * NB + 4, NJ_S = (4 * NB + 15) / 16;
            float* const slab = g.C + (int64_t)split * g.slab_stride;
#pragma unroll
            for (int i = 0; i < TMB; ++i) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int t = 0; t < 4; ++t) lds[(4 * q + t) * LDS_S + 16 * b + r] = acc[i][b][t];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int p4 = 0; p4 < 4; ++p4) {
                    const int m = m0 + 16 * i + 4 * p4 + q;
#pragma unroll
                    for (int j = 0; j < NJ_S; ++j) {
                        const int c4 = r + 16 * j;
                        const int n = n0 + 4 * c4;
                        const f32x4 v = *reinterpret_cast<const f32x4*>(lds + (4 * p4 + q) * LDS_S + 4 * min(c4, 4 * NB - 1));
                        if (c4 < 4 * NB && m < g.M) {
                            if (n + 3 < g.N) {
                                *reinterpret_cast<f32x4*>(slab + (int64_t)m * g.ldc + n) = v;
                            } else {
                                for (int e = 0; e < 4 && n + e < g.N; ++e) slab[(int64_t)m * g.ldc + n + e] = v[e];
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);  // (the next block's staging writes stay behind this block's reads)
            }
            continue;  // (the fused epilogues below belong to the other instantiations)
        }

        // ---- epilogue: the tile goes through the wave's LDS (the chunk images are dead) one block of 16 rows at a time and leaves
        // in ROWS -- lane (r, q) owns four consecutive columns 4 (r + 16 j) of row 4 p + q: 16-byte accesses, 256 contiguous bytes
        // per row and instruction, 12 stores per row block instead of 44 (and as many target / x_t loads) ----
        constexpr int LDS_ = 16 * NB + 4;  // floats per staged row (+4: the four q groups of a ds_write_b32 hit different banks)
        constexpr int NJ = (4 * NB + 15) / 16;
        typedef f32x4 f32x4_e __attribute__((aligned(4)));
        f32x4 bias4[NJ];
        int col4[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            col4[j] = n0 + 4 * (r + 16 * j);
            bias4[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (g.bias && r + 16 * j < 4 * NB) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bias4[j][e] = g.bias[min(col4[j] + e, g.N - 1)];
            }
        }
        const bool has_z = (EPI == GD_EPI_POST) && (g.aux2 != nullptr);
        const bool has_r = (EPI == GD_EPI_POST) && (g.r2 != nullptr);
        // What a step of four rows reads from global memory -- the rows' coefficients, their targets (LOSS) or x_t / noise (POST) --
        // is fetched ONE STEP AHEAD: the wave is alone on its SIMD, so a load waited for where it is issued stands still for a full
        // memory round trip, twenty times per tile (measured: the posterior product 0.272 ms in the reverse loop).  Rows are clamped
        // into the matrix, the 16-byte groups that do not lie inside it whole (last column tile) are fetched in their own step.
        struct Pre {
            f32x4 a[NJ], z[NJ];
            uint32_t w[NJ];
            float c1, c2, p1, p2, sg;
        } pre[2];
        auto fetch = [&](int i, int p4, Pre& P) {
            const int mc = min(m0 + 16 * i + 4 * p4 + q, g.M - 1);
            P.c1 = 1.f; P.c2 = 0.f; P.p1 = 0.f; P.p2 = 0.f; P.sg = 0.f;
            if (EPI == GD_EPI_LOSS) {
                if (g.r0) P.c1 = g.r0[mc];
            } else {
                P.c1 = g.r0[mc];
                P.c2 = g.r1[mc];
                if (has_r) { P.p1 = g.r2[mc]; P.p2 = g.r3[mc]; }
                if (has_z) P.sg = g.r4[mc];
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int n = col4[j];
                const bool whole = (r + 16 * j < 4 * NB) && n + 3 < g.N;  // (row clamped: the address is valid whatever m is)
                P.w[j] = 0u;
                P.a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                P.z[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (EPI == GD_EPI_LOSS && g.aux_bits) {
                    P.w[j] = g.aux_bits[(int64_t)mc * g.ldbits + min((int64_t)(n >> 5), g.ldbits - 1)];
                } else if (whole) {
                    P.a[j] = *reinterpret_cast<const f32x4_e*>(g.aux + (int64_t)mc * g.ldaux + n);
                    if (has_z) P.z[j] = *reinterpret_cast<const f32x4_e*>(g.aux2 + (int64_t)mc * g.ldaux2 + n);
                }
            }
        };
        fetch(0, 0, pre[0]);
#pragma unroll
        for (int i = 0; i < TMB; ++i) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t) lds[(4 * q + t) * LDS_ + 16 * b + r] = acc[i][b][t];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int p4 = 0; p4 < 4; ++p4) {
                const int step = 4 * i + p4;
                const Pre& P = pre[step & 1];
                if (step + 1 < 4 * TMB) fetch((step + 1) >> 2, (step + 1) & 3, pre[(step + 1) & 1]);
                const int m = m0 + 16 * i + 4 * p4 + q;
                const int mc = min(m, g.M - 1);
                const bool mok = m < g.M;
                float ss = 0.f;
                const float c1 = P.c1, c2 = P.c2, p1 = P.p1, p2 = P.p2, sg = P.sg;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int c4 = r + 16 * j;
                    const bool inb = c4 < 4 * NB;                      // inside the tile
                    const int n = col4[j];
                    const bool whole = inb && n + 3 < g.N;             // a whole 16-byte group inside the matrix's columns
                    const bool full = whole && mok;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(lds + (4 * p4 + q) * LDS_ + 4 * min(c4, 4 * NB - 1));
                    f32x4 o, o2 = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (EPI == GD_EPI_LOSS) {
                        // d = alpha * (acc + bias) - target, stored; per-row sum of d^2 (gaussian_diffusion.py:335)
                        f32x4 tg;
                        if (g.aux_bits) {  // {0,1} target rows as bitmaps: four bits of one word (n is a multiple of 4)
                            const uint32_t w = P.w[j] >> (n & 31);
#pragma unroll
                            for (int e = 0; e < 4; ++e) tg[e] = (float)((w >> e) & 1u);
                        } else if (whole) {
                            tg = P.a[j];
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) tg[e] = g.aux[(int64_t)mc * g.ldaux + min(n + e, g.N - 1)];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            o2[e] = v[e] + bias4[j][e];
                            o[e] = c1 * o2[e] - tg[e];
                            if (inb && mok && n + e < g.N) ss += o[e] * o[e];
                        }
                    } else {
                        // posterior mean of the reverse step (gaussian_diffusion.py:451-471, :495-498, :210-217)
                        f32x4 xt = P.a[j], zz = P.z[j];
                        if (!whole) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                xt[e] = g.aux[(int64_t)mc * g.ldaux + min(n + e, g.N - 1)];
                                if (has_z) zz[e] = g.aux2[(int64_t)mc * g.ldaux2 + min(n + e, g.N - 1)];
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float vv = v[e] + bias4[j][e];
                            o2[e] = has_r ? (p1 * xt[e] - p2 * vv) : vv;  // pred_xstart
                            o[e] = c1 * o2[e] + c2 * xt[e];
                            if (has_z) o[e] += sg * zz[e];
                        }
                    }
                    if (full) {
                        *reinterpret_cast<f32x4_e*>(g.C + (int64_t)m * g.ldc + n) = o;
                        if (g.out2) *reinterpret_cast<f32x4_e*>(g.out2 + (int64_t)m * g.ldout2 + n) = o2;
                    } else if (inb && mok) {
                        for (int e = 0; e < 4 && n + e < g.N; ++e) {
                            g.C[(int64_t)m * g.ldc + n + e] = o[e];
                            if (g.out2) g.out2[(int64_t)m * g.ldout2 + n + e] = o2[e];
                        }
                    }
                }
                if (EPI == GD_EPI_LOSS) {
                    ss += __shfl_xor(ss, 1);
                    ss += __shfl_xor(ss, 2);
                    ss += __shfl_xor(ss, 4);
                    ss += __shfl_xor(ss, 8);
                    if (r == 0 && mok) g.rowpart[(int64_t)m * g.ld_rowpart + tn] = ss;
                }
                __builtin_amdgcn_sched_barrier(0);  // four rows at a time: keeps the epilogue's live registers bounded
            }
        }
    }
}

template <int NB>
int dr_fat_go(const DrArgs& d, int epi, int dma, int n_cu, hipStream_t s) {
    const size_t lds = (size_t)4 * 2 * NB * 256 * sizeof(float) + 4 * 64 * sizeof(float);  // chunk images + a scratch line per wave (x_t prefetch)
    void (*kern)(const DrArgs) =
        dma ? (epi == GD_EPI_SLAB ? dr_fat_kernel<NB, GD_EPI_SLAB, 1> : epi == GD_EPI_LOSS ? dr_fat_kernel<NB, GD_EPI_LOSS, 1> : dr_fat_kernel<NB, GD_EPI_POST, 1>)
            : (epi == GD_EPI_SLAB ? dr_fat_kernel<NB, GD_EPI_SLAB, 0> : epi == GD_EPI_LOSS ? dr_fat_kernel<NB, GD_EPI_LOSS, 0> : dr_fat_kernel<NB, GD_EPI_POST, 0>);
    static bool attr_set[6] = {false, false, false, false, false, false};
    const int ai = epi == GD_EPI_SLAB ? 4 + dma : 2 * dma + (epi == GD_EPI_LOSS);
    if (!attr_set[ai] && lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            gdmcf_set_error("hipFuncSetAttribute(dr_fat_kernel, LDS=%zu): %s", lds, hipGetErrorString(e));
            return GDMCF_E_HIP;
        }
        attr_set[ai] = true;
    }
    hipLaunchKernelGGL(kern, dim3(n_cu), dim3(256), lds, s, d);
    return GDMCF_OK;
}

// B's pieces straight into LDS (GDMCF_FAT_DMA=1; 0: through staging registers): 16 bytes per lane from a 16-byte-aligned source,
// any other weight runs the register-staged loop
int dr_fat_dma(const GdGemm& g) {
    static const int dma_env = gd_env_int("GDMCF_FAT_DMA", GD_FAT_DMA_DEFAULT);
    return (dma_env > 0 && (reinterpret_cast<uintptr_t>(g.B) & 15) == 0 && (g.ldb & 3) == 0) ? 1 : 0;
}

}  // namespace

// The output layer with a fused epilogue as ONE FAT TILE PER WAVE, or GD_DR_NOT_TAKEN with g as it was.
int gd_dr_fat_launch(int epi, GdGemm& g, hipStream_t s) {
    if (!dr_routes().fat) return GD_DR_NOT_TAKEN;
    const int64_t lim = (int64_t)1 << 32;  // 32-bit byte offsets inside every matrix
    const int n_cu = dr_cu_count();
    const int tiles_m = gd_cdiv(g.M, 80);
    bool ok = (int64_t)g.M * g.lda * 4 < ((int64_t)1 << 31) && (int64_t)g.N * g.ldb * 4 < lim && g.lda >= g.K && g.ldb >= g.K &&
              g.K >= 256 && (long)tiles_m * 80 * 100 <= (long)g.M * 112 &&  // 80-row tiles: at most 12 % padding
              (n_cu & 7) == 0 && !(epi == GD_EPI_LOSS && g.rowpart == nullptr) &&
              !(epi == GD_EPI_LOSS && g.aux_bits && g.ldbits < (g.N + 31) / 32);
    // width of the tile: the one whose rounds of one tile per SIMD cost the least matrix time (rounds x NB)
    int nb = 0;
    long best = 1L << 60;
    const long slots = 4L * n_cu;
    for (int c = 12; c >= 8 && ok; --c) {
        const long t = (long)tiles_m * gd_cdiv(g.N, 16 * c);
        const long cost = ((t + slots - 1) / slots) * c;
        if (t >= slots / 2 && cost < best) { best = cost; nb = c; }
    }
    if (ok && epi == GD_EPI_POST) {
        // the reverse step reads x_t and writes x_{t-1} in the epilogue (2 x 4 B per element): with every wave finishing at once
        // that burst runs under nothing, so this kernel only takes the product when the LDS-tiled kernel's last round of
        // workgroups would be badly filled (measured: Yelp width 0.248 against 0.267 ms, Amazon-Book width 0.706 against 0.663)
        const long t128 = (long)gd_cdiv(g.M, 80) * gd_cdiv(g.N, 128);
        const long rounds = (t128 + 2 * n_cu - 1) / (2 * n_cu);
        if (t128 * 100 >= rounds * 2 * n_cu * 90) ok = false;
    }
    if (!ok || !nb || (epi == GD_EPI_LOSS && g.ld_rowpart < gd_cdiv(g.N, 16 * nb))) return GD_DR_NOT_TAKEN;
    DrArgs d = {};
    d.tiles_m = tiles_m;
    d.tiles_n = gd_cdiv(g.N, 16 * nb);
    d.m_fastest = 1;
    d.ksp = gd_cdiv(g.K, 16);  // chunks of 16 k
    {
        // x_t prefetch of the reverse step: this many chunks before the end of the k loop (0: off; A/B knob)
        static const int pf = gd_env_int("GDMCF_FAT_PF", 10);
        d.stagger = pf;  // (DrArgs: the field doubles as this kernel's prefetch distance)
    }
    const int dma = dr_fat_dma(g);
    g.tiles_m = d.tiles_m;
    g.tiles_n = d.tiles_n;
    d.g = g;
    d.ctr = 0;
    int rc = GDMCF_OK;
    {
        GdProfScope prof(g.prof_tag, 2.0 * g.M * g.N * g.K, s);
        switch (nb) {
            case 8: rc = dr_fat_go<8>(d, epi, dma, n_cu, s); break;
            case 9: rc = dr_fat_go<9>(d, epi, dma, n_cu, s); break;
            case 10: rc = dr_fat_go<10>(d, epi, dma, n_cu, s); break;
            case 11: rc = dr_fat_go<11>(d, epi, dma, n_cu, s); break;
            default: rc = dr_fat_go<12>(d, epi, dma, n_cu, s); break;
        }
    }
    if (rc != GDMCF_OK) return rc;
    t_gd_last_gemm = 4;
    return gd_launch_status("gemm_dr");
}

// Tile width, split count and chunks per split of the first-layer forward on dr_fat_kernel<NB, GD_EPI_SLAB, 1> (common.h).  One
// (split, tile) task per wave slot, one round: for every width the splits that fill the slots (at least eight chunks each, at most
// 64 slabs for the reducer to sum), and of the widths the one whose task costs the least matrix time, NB x chunks per split.
int gd_dr_fat_slab_plan(int M, int N, int K, int* nb_out, int* cps_out) {
    if (!dr_routes().fat_slab || M <= 0 || N < 128 || K < 4096) return 0;
    const int n_cu = dr_cu_count();
    const int tiles_m = gd_cdiv(M, 80);
    if ((n_cu & 7) != 0 || (long)tiles_m * 80 * 100 > (long)M * 112) return 0;  // 80-row tiles: at most 12 % padding
    const long slots = 4L * n_cu;
    const int chunks = gd_cdiv(K, 16);
    int nb = 0, cps = 0;
    long best = 1L << 60;
    for (int c = 8; c <= 12; ++c) {
        const long tiles = (long)tiles_m * gd_cdiv(N, 16 * c);
        if (tiles > slots) continue;
        long sp = slots / tiles;
        if (sp > chunks / 8) sp = chunks / 8;
        if (sp > 64) sp = 64;
        if (sp < 2) continue;
        const int per = gd_cdiv(chunks, (int)sp);
        if ((long)c * per < best) { best = (long)c * per; nb = c; cps = per; }
    }
    if (!nb) return 0;
    if (nb_out) *nb_out = nb;
    if (cps_out) *cps_out = cps;
    return gd_cdiv(chunks, cps);  // (the real split count: the last split may be short, none is empty)
}

// The first-layer forward xin W1^T (both operands K-contiguous) as split-K slabs on the fat-tile loop (sets g.splits / kchunk / tiles_*
// for the reducer), or GD_DR_NOT_TAKEN with g as it was.  A weight that is not 16-byte aligned (a contiguous nn.Linear weight with
// an odd K) runs the register-staged loop on the same plan: same MFMAs, same k order, same slabs -- the layer's result does not
// depend on where its weight's rows are seated (tests/test_gpu_dw_multi.py compares a seated weight with a contiguous one bit for bit).
int gd_dr_fat_slab_launch(GdGemm& g, hipStream_t s) {
    int nb = 0, cps = 0;
    const int splits = gd_dr_fat_slab_plan(g.M, g.N, g.K, &nb, &cps);
    if (!splits) return GD_DR_NOT_TAKEN;
    const size_t need = (size_t)splits * g.M * g.ldc * sizeof(float);
    const bool ok = gd_aligned16(g.C) && (g.ldc & 3) == 0 && g.ldc >= g.N &&
                    g.ws_cap >= need && g.slab_stride >= (int64_t)g.M * g.ldc && (g.slab_stride & 3) == 0 &&
                    (int64_t)g.M * g.lda * 4 < ((int64_t)1 << 31) && (int64_t)g.N * g.ldb * 4 < ((int64_t)1 << 32) && g.lda >= g.K && g.ldb >= g.K;
    if (!ok) return GD_DR_NOT_TAKEN;
    const int n_cu = dr_cu_count();
    DrArgs d = {};
    d.tiles_m = gd_cdiv(g.M, 80);
    d.tiles_n = gd_cdiv(g.N, 16 * nb);
    d.m_fastest = 1;
    d.ksp = gd_cdiv(g.K, 16);  // chunks of 16 k in the whole reduction; a task runs g.kchunk / 16 of them
    g.splits = splits;
    g.kchunk = cps * 16;
    g.tiles_m = d.tiles_m;
    g.tiles_n = d.tiles_n;
    d.g = g;
    d.ctr = 0;
    const int dma = dr_fat_dma(g);
    int rc = GDMCF_OK;
    {
        GdProfScope prof(g.prof_tag, 2.0 * g.M * g.N * g.K, s);
        switch (nb) {
            case 8: rc = dr_fat_go<8>(d, GD_EPI_SLAB, dma, n_cu, s); break;
            case 9: rc = dr_fat_go<9>(d, GD_EPI_SLAB, dma, n_cu, s); break;
            case 10: rc = dr_fat_go<10>(d, GD_EPI_SLAB, dma, n_cu, s); break;
            case 11: rc = dr_fat_go<11>(d, GD_EPI_SLAB, dma, n_cu, s); break;
            default: rc = dr_fat_go<12>(d, GD_EPI_SLAB, dma, n_cu, s); break;
        }
    }
    if (rc != GDMCF_OK) return rc;
    t_gd_last_gemm = 6;
    return gd_launch_status("gemm_dr_fat_slab");
}
