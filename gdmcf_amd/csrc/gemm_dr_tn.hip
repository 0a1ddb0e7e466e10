// The register-streaming weight-gradient kernels of gemm_dr.h: dr_tn_kernel and dr_tn_adamw_kernel (they share the ticket counters,
// hence the file), their launchers, and the two entry points gd_dr_tn_launch / gd_gemm_dr_adamw_multi.
//
// Row-contiguous operand P[k][rows] (the weight-gradient products, reference main.py:350 / models/DNN.py:79-86): one
// buffer_load_dwordx4 per wave brings rows r0 .. r0+63 of four consecutive k; lane (i = lane & 15, q = lane >> 4) holds
// P[k0 + q][r0 + 4 i + e], e = 0..3, and register e IS the operand of the MFMA block whose 16 rows are r0 + 4 i + e (any
// fixed assignment of matrix rows to MFMA rows is as good as another).  256 contiguous bytes per lane group, nothing to
// transpose.  With both operands loaded this way the accumulators hold
//     acc[a][e][b][f][t] = C[m0 + 64 a + 16 q + 4 t + e][n0 + 64 b + 4 r + f],   r = lane & 15, q = lane >> 4,
// i.e. four consecutive columns (f) per lane and 256 contiguous bytes per row and store instruction.
//
// Pipeline (per wave): a ring of R = D + 1 register slots, one k-step (4 k) each.  While step s is multiplied, the loads of
// step s + D are issued BETWEEN its MFMAs into the slot step s - 1 has just left; every step waits with the same counted
// s_waitcnt vmcnt.  Loads go through raw buffer descriptors (base + per-lane voffset + scalar soffset): advancing a k-step is
// one scalar add, and anything outside the matrix returns 0 instead of faulting (K tails, steps past the end).  The ring runs
// CONTINUOUSLY across tiles -- during the last D steps of a tile the loads already belong to the next tile, whose id comes
// from a ticket drawn one tile earlier -- so a tile boundary costs neither a pipeline fill nor a drain; a tile runs a
// multiple of R steps so that slot indices stay compile-time constants.  Two waves share a SIMD (one 512-thread workgroup
// per CU); the hardware prefers the older one, which starves the younger and leaves a long tail, so a wave raises its
// priority with the progress of its tile (s_setprio): the tile closest to its end wins.
//
// Determinism: the tile -> wave assignment is dynamic, the arithmetic of a tile is not (fixed k order, one wave per tile):
// results are bit-identical from run to run.
#include <stdlib.h>

#include <atomic>

#include "gemm_dr.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ticket counters: one SET per launch in flight (dr_ticket_slot below), one queue per XCD inside a set, each on a 128-byte line of
// its own; a queue's last draw resets it, so every set is zero again when its launch has drained
__device__ unsigned int g_dr_ticket[32][8][32];

__device__ __forceinline__ i32x4 dr_srd(const void* p, uint32_t bytes) {
    const uint64_t a = (uint64_t)p;
    return i32x4{(int)(uint32_t)a, (int)((uint32_t)(a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

// ring loads are asm: hipcc neither counts nor waits for them, the kernel places the counted s_waitcnt itself
__device__ __forceinline__ f32x4 dr_load(i32x4 srd, uint32_t voff, uint32_t soff) {
    f32x4 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(srd), "s"(soff) : "memory");
    return v;
}

template <int N>
__device__ __forceinline__ void dr_wait() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// lane 0 draws a ticket.  The returning atomic is asm so that hipcc does not wait for it on the spot: it is older than
// every ring load of the tile it is issued in and has long landed when the cursor leaves that tile.
__device__ __forceinline__ unsigned int dr_ticket_issue(unsigned int* ctr) {
    unsigned int t;
    unsigned long long save;
    const unsigned int zero = 0, one = 1;
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %2, %3, %4 sc0\n\ts_mov_b64 exec, %1"
                 : "=&v"(t), "=&s"(save) : "v"(zero), "v"(one), "s"(ctr) : "memory");
    return t;
}

#ifndef GD_ADAMW_DBG
#define GD_ADAMW_DBG 0
#endif

// One weight-gradient product with its AdamW update, as dr_tn_adamw_kernel takes it: C = W[M, N] = A[K, M]^T B[K, N] (N counts
// the bias column when there is one), exp_avg / exp_avg_sq beside W with W's leading dimension.
struct DrAdamProd {
    const float* A;
    const float* B;
    float* W;
    float* ea;    // exp_avg
    float* ea2;   // exp_avg_sq
    float* bias;  // bias gradient (column N - 1 of the product), or NULL
    int lda, ldb, ldc;
    int M, N, K;
    int tiles_m, tiles_n, m_fastest;
    const GdAdamHyper* adam_dev;  // this step's scalars in device memory (graph replay), NULL = adam
    GdAdamHyper adam;
};
constexpr int DR_MULTI_MAX = 4;
// Several such products in ONE launch: one tile queue over all of them (a queue serves its panels of product 0, then of product
// 1, ...), so the launch has one ramp, one final stream drain and one ragged last round however many products it holds.  Every
// product runs the same k-steps per tile (the same reduction length: the batch).
struct DrMultiArgs {
    DrAdamProd p[DR_MULTI_MAX];
    int n;        // products
    int ksp;      // k-steps run per tile (a multiple of the ring size)
    int ctr;      // index into g_dr_ticket
    int stagger;  // waves 4-7 of a workgroup start this many x 3.4 us later
};

// C[M,N] = A[K,M]^T * B[K,N], both operands row-contiguous.  TA / TB: 64-row load units per operand and k-step.
// (The fused-AdamW form of this product: dr_tn_adamw_kernel.)
template <int TA, int TB, int D>
__global__ __launch_bounds__(512, 2) void dr_tn_kernel(const DrArgs d) {
    constexpr int LPS = TA + TB;  // loads per k-step
    constexpr int R = D + 1;
    static_assert(LPS * D <= 63, "vmcnt is a 6-bit counter");
    const GdGemm& g = d.g;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    // ---- tiles and tickets.  "Panel" = the tiles that share a 64-row slice of the LARGER operand; the panels p with p % 8 == x
    // form queue x, served first by the waves that run on XCD x (HW_REG_XCC_ID): a panel's slice is then fetched into ONE L2
    // instead of eight (measured before: 325 MB fetched per launch for 57 MB of operands).  A wave that finds its queue empty
    // goes on to the next one, so the queues only set who takes what first, never who may take what (placement-independent).
    // Ticket t of queue x = tile (t % minor) of its panel (t / minor).  Every wave draws from a queue until a draw fails, i.e.
    // fails exactly once per queue: a queue of n tiles sees n + n_waves draws per launch and the last draw resets it.
    const int n_waves = gridDim.x * 8;
    const int minor = d.m_fastest ? d.tiles_m : d.tiles_n;   // tiles per panel
    const int panels = d.m_fastest ? d.tiles_n : d.tiles_m;
    int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    int qx = xcc & 7;                                         // queue being drawn from
    int visited = 0;                                          // queues this wave has exhausted
    auto q_tiles = [&](int x) { return ((panels - x + 7) >> 3) * minor; };
    auto tile_of = [&](int x, int t) {                        // -> tile id in the (m_fastest ? tn * tiles_m + tm : tm * tiles_n + tn) numbering
        const int p = (t / minor) * 8 + x, i = t % minor;
        return p * minor + i;
    };
    // draw (blocking) until a queue yields a tile or all eight have failed; returns -1 when the wave is done
    auto draw_blocking = [&]() {
        for (;;) {
            if (visited == 8) return -1;
            unsigned int* c = &g_dr_ticket[d.ctr][qx][0];
            unsigned int tk = dr_ticket_issue(c);
            dr_wait<0>();
            asm volatile("" : "+v"(tk));
            const int t = __builtin_amdgcn_readfirstlane(tk);
            const int n = q_tiles(qx);
            if (t == n + n_waves - 1 && lane == 0) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t < n) return tile_of(qx, t);
            qx = (qx + 1) & 7;
            ++visited;
        }
    };
    if (d.stagger > 0 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
        for (int i = 0; i < d.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    int cur = draw_blocking();
    if (cur < 0) return;
    const int ntiles = d.tiles_m * d.tiles_n;
    const int KSP = d.ksp;
    // the descriptors end with the last valid element: rows k >= K and everything behind the matrices reads as 0
    const i32x4 srdA = dr_srd(g.A, (uint32_t)(((int64_t)(g.K - 1) * g.lda + g.M) * 4));
    const i32x4 srdB = dr_srd(g.B, (uint32_t)(((int64_t)(g.K - 1) * g.ldb + g.N) * 4));
    const uint32_t sa = 16u * (uint32_t)g.lda, sb = 16u * (uint32_t)g.ldb;
    // (with a bias column the product has one more column than C: the descriptor ends with C's own last element, or the first
    // lane of the row tile past M would pass the range check by that one element)
    const uint32_t c_bytes = (uint32_t)(((int64_t)(g.M - 1) * g.ldc + (g.out2 ? g.N - 1 : g.N)) * 4);
    const __amdgpu_buffer_rsrc_t srdC = __builtin_amdgcn_make_buffer_rsrc(g.C, 0, (int)c_bytes, 0x00020000);

    // ---- load cursor: the tile whose operands are being fetched ----
    uint32_t offA[TA], offB[TB];  // per-lane byte offsets inside the cursor's tile
    uint32_t ka = 0, kb = 0;      // byte offset of the k-step to load next (soffset operand)
    int l_left = KSP;             // steps of the cursor's tile not yet issued
    auto set_cursor = [&](int tile) {
        const bool ok = tile < ntiles;  // past the end the cursor is parked outside both matrices: every load returns 0
        const int tm = d.m_fastest ? (tile % d.tiles_m) : (tile / d.tiles_n);
        const int tn = d.m_fastest ? (tile / d.tiles_m) : (tile % d.tiles_n);
#pragma unroll
        for (int a = 0; a < TA; ++a) offA[a] = ok ? (uint32_t)(q * g.lda + tm * (64 * TA) + 64 * a + 4 * r) * 4u : 0xFFFFFFF0u;
#pragma unroll
        for (int b = 0; b < TB; ++b) offB[b] = ok ? (uint32_t)(q * g.ldb + tn * (64 * TB) + 64 * b + 4 * r) * 4u : 0xFFFFFFF0u;
        ka = kb = 0;
        l_left = KSP;
    };
    set_cursor(cur);
    f32x4 ra[R][TA], rb[R][TB];
#pragma unroll
    for (int u = 0; u < D; ++u) {
#pragma unroll
        for (int a = 0; a < TA; ++a) ra[u][a] = dr_load(srdA, offA[a], ka);
#pragma unroll
        for (int b = 0; b < TB; ++b) rb[u][b] = dr_load(srdB, offB[b], kb);
        ka += sa;
        kb += sb;
        --l_left;
    }
    const int q1 = (KSP / R / 4) * R, q2 = (KSP / R / 2) * R, q3 = (KSP / R * 3 / 4) * R;
    for (;;) {
        // the ticket of the tile AFTER this one travels under this tile's work (needed when the cursor leaves this tile)
        unsigned int* tctr = &g_dr_ticket[d.ctr][qx][0];
        unsigned int tick = visited < 8 ? dr_ticket_issue(tctr) : 0u;
        const bool drew = visited < 8;
        int nxt = 0;
        const int tm = d.m_fastest ? (cur % d.tiles_m) : (cur / d.tiles_n);
        const int tn = d.m_fastest ? (cur / d.tiles_m) : (cur % d.tiles_n);
        const int m0 = tm * 64 * TA, n0 = tn * 64 * TB;
        f32x4 acc[TA][4][TB][4];
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < TB; ++b)
#pragma unroll
                    for (int f = 0; f < 4; ++f) acc[a][e][b][f] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_s_setprio(0);
        for (int s0 = 0; s0 < KSP; s0 += R) {
            if (s0 == q1) __builtin_amdgcn_s_setprio(1);
            else if (s0 == q2) __builtin_amdgcn_s_setprio(2);
            else if (s0 == q3) __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                constexpr int NM = 16 * TA * TB;  // MFMAs of this step; the LPS loads ride behind MFMA 2, 6, 10, ...
                const int v = (u + D) % R;        // slot of step s + D (= the slot step s - 1 has left)
                dr_wait<LPS*(D - 1)>();           // step s has landed; steps s+1 .. s+D-1 stay in flight
#pragma unroll
                for (int a = 0; a < TA; ++a) asm volatile("" : "+v"(ra[u][a]));
#pragma unroll
                for (int b = 0; b < TB; ++b) asm volatile("" : "+v"(rb[u][b]));
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    const int a = i / (16 * TB), e = (i / (4 * TB)) % 4, b = (i / 4) % TB, f = i % 4;
                    acc[a][e][b][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[u][a][e], rb[u][b][f], acc[a][e][b][f], 0, 0, 0);
                    if (i % 4 == 1 && i / 4 < LPS) {
                        __builtin_amdgcn_sched_barrier(0);
                        const int l = i / 4;
                        if (l < TA) ra[v][l] = dr_load(srdA, offA[l], ka);
                        else rb[v][l - TA] = dr_load(srdB, offB[l - TA], kb);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (i == 4 * LPS + 1) {
                        __builtin_amdgcn_sched_barrier(0);
                        ka += sa;
                        kb += sb;
                        if (--l_left == 0) {  // once per tile: the cursor moves on to the next tile
                            // the ticket was issued at step 0 of this tile: it is older than every load the counted waits leave
                            // in flight once D - 1 later steps have issued theirs, i.e. when the tile runs >= 2 D steps
                            nxt = -1;
                            if (drew) {
                                if (KSP < 2 * D + 2) dr_wait<0>();
                                asm volatile("" : "+v"(tick));
                                const int tk = __builtin_amdgcn_readfirstlane(tick);
                                const int nq = q_tiles(qx);
                                if (tk == nq + n_waves - 1 && lane == 0) __hip_atomic_store(tctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (tk < nq) {
                                    nxt = tile_of(qx, tk);
                                } else {  // this queue is empty (a few times per wave, at the end of the launch): try the others
                                    qx = (qx + 1) & 7;
                                    ++visited;
                                    nxt = draw_blocking();
                                }
                            }
                            if (nxt < 0) nxt = ntiles;  // parks the cursor
                            set_cursor(nxt);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- epilogue: 16 bytes per lane along N; the row part of the address is scalar (soffset); rows past M fall outside
        // the descriptor, columns past N are cut by the lane ----
#pragma unroll
        for (int b = 0; b < TB; ++b) {
            const int n = n0 + 64 * b + 4 * r;
            const uint32_t vo = (uint32_t)(16 * q * g.ldc + n) * 4u;
            if (n + 3 < (g.out2 ? g.N - 1 : g.N)) {  // (a bias column, the last one, never goes out with a 16-byte group)
                // The row offset travels in the VGPR offset, the scalar offset field stays 0.  With an SGPR there hipcc emits
                // `buffer_store_dwordx4 v[146:149], v0, s[36:39], s10 offen` and refills v146..149 for the next row in the very
                // next instruction: LLVM's hazard recognizer holds that a store of more than 64 bits needs no wait state before
                // its data registers are rewritten when soffset is a register -- on gfx950 it does: lanes 12-15 of every
                // 16-lane row of the FIRST data register went out with the next row's values, in timing-dependent launches
                // (DESIGN 4.1b).  With soffset = 0 the recognizer inserts the s_nop itself.
#pragma unroll
                for (int a = 0; a < TA; ++a)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            f32x4 gv = {acc[a][e][b][0][t], acc[a][e][b][1][t], acc[a][e][b][2][t], acc[a][e][b][3][t]};
                            const uint32_t so = (uint32_t)(m0 + 64 * a + 4 * t + e) * (uint32_t)g.ldc * 4u;
                            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, gv), srdC, vo + so, 0, 0);
                        }
            } else if (n < g.N) {  // the lane's four columns straddle N (last column tile only)
                for (int a = 0; a < TA; ++a)
                    for (int t = 0; t < 4; ++t)
                        for (int e = 0; e < 4; ++e) {
                            const int m = m0 + 64 * a + 16 * q + 4 * t + e;
                            if (m >= g.M) continue;
                            for (int k = 0; k < 4; ++k) {
                                if (n + k >= g.N) continue;
                                const float gk = acc[a][e][b][k][t];
                                if (g.out2 && n + k == g.N - 1) g.out2[m] = gk;  // the bias column (operand B's extra column): its own vector
                                else g.C[(int64_t)m * g.ldc + n + k] = gk;
                            }
                        }
            }
        }
        if (nxt >= ntiles) break;
        cur = nxt;
    }
    // the parked cursor's loads are still in flight: their destination registers stay live (and untouched by the compiler)
    // until they have landed -- a register hipcc believes dead and reuses would be overwritten by such a load
    dr_wait<0>();
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
        for (int a = 0; a < TA; ++a) asm volatile("" ::"v"(ra[u][a]));
#pragma unroll
        for (int b = 0; b < TB; ++b) asm volatile("" ::"v"(rb[u][b]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The weight-gradient product with the AdamW update of that weight in the SAME kernel (reference main.py:350-351:
// loss.backward(); optimizer.step()), single GPU: G = A^T B never reaches memory, W / exp_avg / exp_avg_sq are read and written
// once -- 24 B per parameter instead of 32 + the separate pass.
//
// Round 3 ran the update as the tile's epilogue.  Measured in round 4 (tools/fused_probe.py): the optimiser stream of the
// launch (826 MB at the Yelp shape) then runs at the full HBM rate -- and the matrix pipe stands still meanwhile: fused time =
// matrix time + stream time for every reduction length (0.089 + 0.129 ms at K = 128, 0.215 + 0.110 ms at K = 400), i.e. no
// overlap at all, with one memory round trip per row group or with several in flight alike.  All waves reach their
// epilogues in phase (same tile length everywhere), the burst saturates HBM, and the waves that should multiply meanwhile wait
// for operands behind it (vmcnt retires in order; the per-CU memory pipeline queues their L2 hits behind the misses).
//
// Here the stream of tile i runs INSIDE the k loop of tile i + 1 of the same wave, at a fixed pace: the finished tile is parked
// in LDS (16 KB per wave, wave-private: no barrier), and every ring round (R k-steps) updates two of its sixteen row groups
// (4 rows x 256 B of each of the three arrays): the three loads of a group are issued between the MFMAs of one k-step and
// consumed four steps later -- gradient from LDS, update, three stores.  The traffic is spread evenly over the matrix time of
// every wave (3.8 TB/s for the Yelp weights, 60 % of what HBM sustains), no bursts, whatever the phases of the waves.
//
// Everything vector-memory in the loop is inline asm with hand-counted waits (as the operand ring): hipcc's own counted waits see
// only its own instructions (guide 5.7).  vmcnt retires in order, so the extra instructions only shift the counts: the top-of-step
// wait allows 2 (D - 1) ring loads + the 12 optimiser instructions of a round minus those of the step itself, and the stream's
// instructions are issued ALWAYS -- parked outside the descriptor (loads return 0 without a fetch, stores are dropped) while no
// tile is pending -- so that the counts are the same in every round; the ring fill issues the parked instructions a previous
// round would have issued.  build.py:lint_vmcnt verifies every count and that nothing touches a register in flight.
// (A wave-specialised form -- eight multiplying waves + four stream waves per CU, hand-over through LDS, so that the stream's HBM
// accesses do not sit in the multiplying waves' in-order vmcnt -- was built and measured in round 4: bit-identical, and 0.02-0.03 ms
// SLOWER per launch; with its stream parked it costs only +0.015 ms over the plain product, so what the real stream costs is memory-
// system contention, not the counter.  profiles/r04_fused_stream_ablations.txt, section G.)
// Tiles whose lanes do not all own a full 16-byte group (the last column panel when N % 64 != 0, or with the bias column) are
// updated on the spot from the accumulators, as in round 3 (1/16 of the Yelp output-layer tiles, 1/538 of the first layer's).
//
// One launch takes up to DR_MULTI_MAX products (DrMultiArgs; a single product is the one-element case).  A launch pays at its
// ends: each wave's first tile runs with no stream beside it, its last tile's stream runs after the k loops with the matrix pipe
// idle, and the last round of tiles is ragged.  With all products behind one queue those ends are paid once: the last tile of
// product p a wave draws is streamed inside the k loop of its first tile of product p + 1.  The tile a virtual id names
// (dr_vtile) carries its product, so the three kinds of per-tile state each follow their own tile -- the load cursor's operand
// descriptors, the k loop's tile (its end-of-tile path), and the pending tile's W / moment descriptors and AdamW scalars.
// ---------------------------------------------------------------------------------------------------------------------
#ifdef GD_NO_SNOP  // (probe builds only: the build's lint rejects the kernel without the guard)
#define GD_SNOP ""
#else
#define GD_SNOP "s_nop 4\n\t"
#endif
#ifndef GD_ADAMW_ST
#define GD_ADAMW_ST 1  // cache policy of the optimiser stream's stores: 1 = nt (0 default, 2 sc1, 3 sc0 sc1: probe builds)
#endif
__device__ __forceinline__ void dr_store(f32x4 v, i32x4 srd, uint32_t voff) {
    // (trailing s_nop: a store of more than 64 bits reads its data registers after issue; hipcc cannot see that this is a store.
    // Leading s_nop 4: with ~100 live scalars hipcc keeps descriptors in VGPR lanes and restores them with v_readlane right in
    // front of the statement; an SGPR written by a VALU instruction must not be read by a vector-memory one for 5 wait states)
#if GD_ADAMW_ST == 1
    asm volatile(GD_SNOP "buffer_store_dwordx4 %0, %1, %2, 0 offen nt\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(srd) : "memory");
#elif GD_ADAMW_ST == 2
    asm volatile(GD_SNOP "buffer_store_dwordx4 %0, %1, %2, 0 offen sc1\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(srd) : "memory");
#elif GD_ADAMW_ST == 3
    asm volatile(GD_SNOP "buffer_store_dwordx4 %0, %1, %2, 0 offen sc0 sc1\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(srd) : "memory");
#else
    asm volatile(GD_SNOP "buffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(srd) : "memory");
#endif
}
// (read-write operand: the destination stays ONE virtual register for the whole kernel, so hipcc has no new value to place at
// every load and no PHI copies to insert at loop back edges -- copies that would move a register whose load is in flight)
// Cache policy of the stream's loads.  NT (non-temporal: the line is not kept in L2) when every 256-byte piece of a row covers
// whole 128-byte lines -- rows of W / exp_avg / exp_avg_sq on 128-byte lines, FusedAdamW.fuse_into_backward seats them so --:
// nothing of a line is left for a neighbouring tile, and the stream stops evicting the operand panels (0.277 -> 0.263 and
// 0.301 -> 0.276 ms for the two Yelp products).  With rows that start anywhere the neighbouring tiles' pieces share their first and
// last line, and a line that is not kept is fetched from HBM twice: 0.32 -> 0.40 ms (profiles/r04_fused_stream_ablations.txt D, I).
#ifndef GD_ADAMW_LD
#define GD_ADAMW_LD 0  // probe builds: policy of the loads when NTL is false (0 default, 1 nt, 2 sc1, 3 sc0 sc1, 4 sc0 sc1 nt)
#endif
template <bool NTL>
__device__ __forceinline__ void dr_load0_rw(f32x4& v, i32x4 srd, uint32_t voff) {
    if constexpr (NTL) {
        asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
        return;
    }
#if GD_ADAMW_LD == 1
    asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
#elif GD_ADAMW_LD == 2
    asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen sc1" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
#elif GD_ADAMW_LD == 3
    asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen sc0 sc1" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
#elif GD_ADAMW_LD == 4
    asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen sc0 sc1 nt" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
#else
    asm volatile(GD_SNOP "buffer_load_dwordx4 %0, %1, %2, 0 offen" : "+v"(v) : "v"(voff), "s"(srd) : "memory");
#endif
}

// virtual tile id of a multi-product launch: the product in bits 24.., the product's own tile number below (numbered as in
// dr_tn_kernel); DR_VT_PARK: no tile
constexpr int DR_VT_SHIFT = 24;
constexpr int DR_VT_PARK = 0x7fffffff;

template <int D, bool NTL>
__global__ __launch_bounds__(512, 2) void dr_tn_adamw_kernel(const DrMultiArgs d) {
    constexpr int LPS = 2;  // ring loads per k-step
    constexpr int R = D + 1;
    // the optimiser stream's schedule inside a ring round: slot A is consumed AND reloaded in step UA, slot B in step UB -- a row
    // group's loads have a whole round (R k-steps, ~4 us with two waves per SIMD) to land
    constexpr int UA = 1, UB = 1 + R / 2;
    constexpr int XS = 6;   // optimiser instructions of such a step: 3 stores + 3 loads
    constexpr int XR = 12;  // ... of a round
    static_assert(UB < R && UB > UA, "two distinct steps of a round");
    static_assert(LPS * R + XS <= 63, "vmcnt is a 6-bit counter");
    constexpr uint32_t PARK = 0xFFFFFF00u;  // outside every descriptor
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    extern __shared__ __attribute__((aligned(16))) float dr_lds[];
    f32x4* const stash = reinterpret_cast<f32x4*>(dr_lds + wave * 4096) + lane;  // [16 accumulators][64 lanes] x 16 B
    // ---- tiles and tickets: as dr_tn_kernel, with the panels of every product behind one another in each queue ----
    const int n_waves = gridDim.x * 8;
    int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    int qx = xcc & 7, visited = 0;
    // (panels dealt round-robin over the queues.  Contiguous blocks of panels per queue -- neighbouring panels on one XCD, close in
    // time, for the 128-byte lines two neighbouring tiles share -- measured slower: 0.314 / 0.327 against 0.293 / 0.318 ms.)
    auto minor_of = [&](int p) { return d.p[p].m_fastest ? d.p[p].tiles_m : d.p[p].tiles_n; };
    auto q_tiles_of = [&](int p, int x) { return (((d.p[p].m_fastest ? d.p[p].tiles_n : d.p[p].tiles_m) - x + 7) >> 3) * minor_of(p); };
    auto q_tiles = [&](int x) {
        int n = 0;
        for (int p = 0; p < d.n; ++p) n += q_tiles_of(p, x);
        return n;
    };
    auto tile_of = [&](int x, int t) {  // ticket t < q_tiles(x) of queue x -> virtual tile id
        int p = 0;
        for (; p < d.n - 1; ++p) {
            const int n = q_tiles_of(p, x);
            if (t < n) break;
            t -= n;
        }
        const int minor = minor_of(p);
        return (p << DR_VT_SHIFT) | (((t / minor) * 8 + x) * minor + t % minor);
    };
    auto tile_mn = [&](int vt, int& tm, int& tn) {
        const DrAdamProd& P = d.p[vt >> DR_VT_SHIFT];
        const int t = vt & ((1 << DR_VT_SHIFT) - 1);
        tm = P.m_fastest ? (t % P.tiles_m) : (t / P.tiles_n);
        tn = P.m_fastest ? (t / P.tiles_m) : (t % P.tiles_n);
    };
    auto draw_blocking = [&]() {
        for (;;) {
            if (visited == 8) return -1;
            unsigned int* c = &g_dr_ticket[d.ctr][qx][0];
            unsigned int tk = dr_ticket_issue(c);
            dr_wait<0>();
            asm volatile("" : "+v"(tk));
            const int t = __builtin_amdgcn_readfirstlane(tk);
            const int n = q_tiles(qx);
            if (t == n + n_waves - 1 && lane == 0) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (t < n) return tile_of(qx, t);
            qx = (qx + 1) & 7;
            ++visited;
        }
    };
    if (d.stagger > 0 && __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
        for (int i = 0; i < d.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    int cur = draw_blocking();
    if (cur < 0) return;
    const int KSP = d.ksp;

    // ---- load cursor: the tile whose operands are being fetched, with its product's operand descriptors ----
    i32x4 srdA, srdB;
    uint32_t sa, sb, offA, offB, ka = 0, kb = 0;
    int l_left = KSP;
    auto set_cursor = [&](int vt) {
        vt = __builtin_amdgcn_readfirstlane(vt);
        const bool ok = vt != DR_VT_PARK;  // parked: outside both matrices (of product 0), every load returns 0
        const int vo = ok ? vt : 0;
        const DrAdamProd& P = d.p[vo >> DR_VT_SHIFT];
        int tm, tn;
        tile_mn(vo, tm, tn);
        srdA = dr_srd(P.A, (uint32_t)(((int64_t)(P.K - 1) * P.lda + P.M) * 4));
        srdB = dr_srd(P.B, (uint32_t)(((int64_t)(P.K - 1) * P.ldb + P.N) * 4));
        sa = 16u * (uint32_t)P.lda;
        sb = 16u * (uint32_t)P.ldb;
        offA = ok ? (uint32_t)(q * P.lda + tm * 64 + 4 * r) * 4u : 0xFFFFFFF0u;
        offB = ok ? (uint32_t)(q * P.ldb + tn * 64 + 4 * r) * 4u : 0xFFFFFFF0u;
        ka = kb = 0;
        l_left = KSP;
    };
    set_cursor(cur);
    // ---- optimiser stream state: the tile parked in LDS with its product's W / exp_avg / exp_avg_sq descriptors and AdamW
    // scalars, its next row group, the two row groups in flight ----
    auto c_bytes_of = [&](int p) {  // (a bias column, the product's last, goes to `bias`: it is not part of W)
        const DrAdamProd& P = d.p[p];
        return (uint32_t)(((int64_t)(P.M - 1) * P.ldc + (P.bias ? P.N - 1 : P.N)) * 4);
    };
    i32x4 srdW, srdM, srdV;
    uint32_t ldc4;
    GdAdamHyper hy;
    int pp;  // the pending tile's product
    auto set_pending_product = [&](int p) {
        p = __builtin_amdgcn_readfirstlane(p);  // (wave-uniform: tells hipcc the descriptors below are scalars)
        const DrAdamProd& P = d.p[p];
        const uint32_t cb = c_bytes_of(p);
        srdW = dr_srd(P.W, cb);
        srdM = dr_srd(P.ea, cb);
        srdV = dr_srd(P.ea2, cb);
        ldc4 = (uint32_t)P.ldc * 4u;
        // this step's AdamW scalars: by value, or -- a step replayed from a hipGraph -- from the device's step state
        hy = P.adam;
        if (P.adam_dev) hy = *P.adam_dev;
        pp = p;
    };
    set_pending_product(cur >> DR_VT_SHIFT);
    uint32_t pend_base = PARK;  // per-lane byte offset of row group 0 of the pending tile inside W / exp_avg / exp_avg_sq
    bool pend_lane = false;     // this lane owns a full 16-byte group in the pending tile (else its stream accesses stay parked)
    int pend_g = 16;            // next row group of the pending tile to issue (16: none left)
    struct Slot {
        f32x4 p, m, v;  // W, exp_avg, exp_avg_sq of the row group in flight
        uint32_t off;   // its per-lane byte offset (PARK: none -- loads return 0 without a fetch, stores are dropped)
        int gi;         // its index: gradient = element gi >> 2 of the parked accumulators 4 (gi & 3) + f
        bool live;      // holds a row group (wave-uniform)
    } sl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        asm volatile("" : "=v"(sl[k].p));
        asm volatile("" : "=v"(sl[k].m));
        asm volatile("" : "=v"(sl[k].v));
        sl[k].off = PARK;
        sl[k].gi = 0;
        sl[k].live = false;
    }
    auto opt_pick = [&](Slot& s_) {  // next row group of the pending tile; parked when there is none
        const bool act = pend_g < 16;
        s_.live = act;
        s_.gi = act ? pend_g : 0;
        s_.off = (act && pend_lane && !(GD_ADAMW_DBG & 2)) ? pend_base + (uint32_t)pend_g * ldc4 : PARK;
        pend_g += act ? 1 : 0;
    };
    auto opt_update_store = [&](Slot& s_) {  // s_.p / m / v have landed
        const float* sg = reinterpret_cast<const float*>(stash + 256 * (s_.gi & 3)) + (s_.gi >> 2);
        float gr[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) gr[f] = sg[256 * f];  // accumulator 4 e + f, element t: 64 lanes x 16 B apart
        f32x4 pn = s_.p, mn = s_.m, vn = s_.v;  // (the slot's registers themselves are only ever written by its loads)
#if !(GD_ADAMW_DBG & 1)  // (probe builds, tools/build_variant.sh: bit 0 = no arithmetic, bit 1 = every stream access parked)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pn[k], mk = mn[k], vk = vn[k];
            gd_adam_elem(pk, gr[k], mk, vk, hy);
            pn[k] = pk;
            mn[k] = mk;
            vn[k] = vk;
        }
#else
        pn[0] += gr[0] + gr[1] + gr[2] + gr[3];
#endif
        // (probe bit 3: stores parked; bit 4: stores go to lines the stream has NOT just loaded -- 448 rows further down)
        const uint32_t so = (GD_ADAMW_DBG & 8) ? PARK : ((GD_ADAMW_DBG & 16) && s_.off != PARK) ? s_.off + 448u * ldc4 : s_.off;
        dr_store(pn, srdW, so);
        dr_store(mn, srdM, so);
        dr_store(vn, srdV, so);
    };
    auto opt_load = [&](Slot& s_) {
        const uint32_t lo = (GD_ADAMW_DBG & 4) ? PARK : s_.off;  // (probe bit 2: loads parked)
        dr_load0_rw<NTL>(s_.p, srdW, lo);
        dr_load0_rw<NTL>(s_.m, srdM, lo);
        dr_load0_rw<NTL>(s_.v, srdV, lo);
    };
    auto opt_pin = [&](Slot& s_) {
        asm volatile("" : "+v"(s_.p));
        asm volatile("" : "+v"(s_.m));
        asm volatile("" : "+v"(s_.v));
    };

    f32x4 ra[R], rb[R];
    // ring fill, with the parked optimiser instructions a previous round would have issued in step u + 1 (see the header)
#pragma unroll
    for (int u = 0; u < D; ++u) {
        ra[u] = dr_load(srdA, offA, ka);
        rb[u] = dr_load(srdB, offB, kb);
        ka += sa;
        kb += sb;
        --l_left;
        const int w = (u + 1) % R;
        if (w == UA || w == UB) {
            // (parked STORES stand in for the loads too: a parked load would still write its destination when it lands, and
            // nothing keeps hipcc from using those registers meanwhile)
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < XS / 3; ++k) {
                dr_store(z, srdW, PARK);
                dr_store(z, srdM, PARK);
                dr_store(z, srdV, PARK);
            }
        }
    }
    const int q1 = (KSP / R / 4) * R, q2 = (KSP / R / 2) * R, q3 = (KSP / R * 3 / 4) * R;
    const bool defer_all = KSP / R >= 9;  // ring rounds per tile: two row groups each, issued in rounds 0..7, consumed by round 8
    for (;;) {
        unsigned int* tctr = &g_dr_ticket[d.ctr][qx][0];
        unsigned int tick = visited < 8 ? dr_ticket_issue(tctr) : 0u;
        const bool drew = visited < 8;
        int nxt = 0;
        int tm, tn;
        tile_mn(cur, tm, tn);
        const int m0 = tm * 64, n0 = tn * 64;
        f32x4 acc[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int f = 0; f < 4; ++f) acc[e][f] = f32x4{0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_s_setprio(0);
        for (int s0 = 0; s0 < KSP; s0 += R) {
            if (s0 == q1) __builtin_amdgcn_s_setprio(1);
            else if (s0 == q2) __builtin_amdgcn_s_setprio(2);
            else if (s0 == q3) __builtin_amdgcn_s_setprio(3);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int v = (u + D) % R;
                // step s has landed; steps s+1 .. s+D-1 and the optimiser instructions of every other step of a round stay in flight
                if (u == UA || u == UB) dr_wait<LPS*(D - 1) + XR - XS>();
                else dr_wait<LPS*(D - 1) + XR>();
                asm volatile("" : "+v"(ra[u]));
                asm volatile("" : "+v"(rb[u]));
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int e = i / 4, f = i % 4;
                    acc[e][f] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[u][e], rb[u][f], acc[e][f], 0, 0, 0);
                    if (i == 1) {
                        __builtin_amdgcn_sched_barrier(0);
                        ra[v] = dr_load(srdA, offA, ka);
                        __builtin_amdgcn_sched_barrier(0);
                    } else if (i == 5) {
                        __builtin_amdgcn_sched_barrier(0);
                        rb[v] = dr_load(srdB, offB, kb);
                        __builtin_amdgcn_sched_barrier(0);
                    } else if (i == 9) {
                        __builtin_amdgcn_sched_barrier(0);
                        ka += sa;
                        kb += sb;
                        if (--l_left == 0) {  // once per tile: the cursor moves on to the next tile
                            nxt = -1;
                            if (drew) {
                                if (KSP < 2 * D + 2) dr_wait<0>();
                                asm volatile("" : "+v"(tick));
                                const int tk = __builtin_amdgcn_readfirstlane(tick);
                                const int nq = q_tiles(qx);
                                if (tk == nq + n_waves - 1 && lane == 0) __hip_atomic_store(tctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (tk < nq) {
                                    nxt = tile_of(qx, tk);
                                } else {
                                    qx = (qx + 1) & 7;
                                    ++visited;
                                    nxt = draw_blocking();
                                }
                            }
                            if (nxt < 0) nxt = DR_VT_PARK;
                            set_cursor(nxt);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    } else if ((u == UA || u == UB) && i == 11) {
                        // ---- the optimiser stream's turn: the slot's row group (loaded one round ago) is updated and stored, and
                        // the slot reloaded with the next row group of the parked tile ----
                        __builtin_amdgcn_sched_barrier(0);
                        Slot& s_ = sl[u == UA ? 0 : 1];
                        // its loads are older than the ring loads of the R steps since (2 each) and the other slot's turn
                        dr_wait<LPS * R + XS>();
                        opt_pin(s_);
                        opt_update_store(s_);
                        opt_pick(s_);
                        opt_load(s_);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- end of tile: the stream's state moves on to this tile's product (the previous pending tile has been consumed in full
        // by a k loop of >= 9 rounds; a shorter loop never leaves one pending) ----
        const int pc = cur >> DR_VT_SHIFT;
        const DrAdamProd& g = d.p[pc];
        set_pending_product(pc);
        const int n_lim = g.bias ? g.N - 1 : g.N;  // columns of W (a bias column, the last one of the product, goes to g.bias)
        const uint32_t vo = (uint32_t)(16 * q * g.ldc + n0 + 4 * r) * 4u;
        const int n = n0 + 4 * r;
        const bool lane_full = n + 3 < n_lim;  // the lane owns a full 16-byte group of every row of the tile
        if (defer_all) {
            // A k loop of >= 9 ring rounds has issued and consumed all sixteen row groups of the PREVIOUS tile (the slots hold
            // parked loads): park this one for the next k loop's stream.  Lanes without a full group (last column panel) stay
            // parked in the stream; what they own is updated element-wise below.
            // (The slots' registers are touched nowhere but in the k loop's turns: any other definition would make hipcc place
            // copies of them -- of registers in flight -- at the loop's back edge.)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int f = 0; f < 4; ++f) stash[64 * (4 * e + f)] = acc[e][f];
            pend_base = vo + (uint32_t)m0 * ldc4;
            pend_lane = lane_full;
            pend_g = 0;
        } else if (lane_full) {
            // a reduction too short for the stream (< 9 ring rounds): updated on the spot from the accumulators, as in round 3
            // (one memory round trip per row group)
            const int c_bytes = (int)c_bytes_of(pc);
            const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(g.W, 0, c_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rM = __builtin_amdgcn_make_buffer_rsrc(g.ea, 0, c_bytes, 0x00020000);
            const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(g.ea2, 0, c_bytes, 0x00020000);
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t o = vo + (uint32_t)(m0 + 4 * t + e) * ldc4;
                    f32x4 pv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, o, 0, 0));
                    f32x4 mv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rM, o, 0, 0));
                    f32x4 vv = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rV, o, 0, 0));
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float pk = pv[k], mk = mv[k], vk = vv[k];
                        gd_adam_elem(pk, acc[e][k][t], mk, vk, hy);
                        pv[k] = pk;
                        mv[k] = mk;
                        vv[k] = vk;
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pv), rW, o, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, mv), rM, o, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, vv), rV, o, 0, 0);
                }
        }
        if (!lane_full && n < g.N) {
            // last column panel: the lane's group straddles the end of the row (N % 4 != 0) or holds the bias column -- element-wise
            // from the accumulators, now (at most one lane per row)
            float* __restrict__ Mo = g.ea;
            float* __restrict__ Vo = g.ea2;
            for (int t = 0; t < 4; ++t)
                for (int e = 0; e < 4; ++e) {
                    const int m = m0 + 16 * q + 4 * t + e;
                    if (m >= g.M) continue;
                    for (int k = 0; k < 4; ++k) {
                        if (n + k >= g.N) continue;
                        const int64_t o = (int64_t)m * g.ldc + n + k;
                        const float gk = acc[e][k][t];
                        if (g.bias && n + k == g.N - 1) {  // the bias column (operand B's extra column): its own vector
                            g.bias[m] = gk;
                            continue;
                        }
                        float pk = g.W[o], mk = Mo[o], vk = Vo[o];
                        gd_adam_elem(pk, gk, mk, vk, hy);
                        g.W[o] = pk;
                        Mo[o] = mk;
                        Vo[o] = vk;
                    }
                }
        }
        if (nxt == DR_VT_PARK) break;
        cur = nxt;
    }
    // the parked cursor's loads and the stream's last instructions are still in flight: their registers stay live until they landed
    dr_wait<0>();
#pragma unroll
    for (int u = 0; u < R; ++u) {
        asm volatile("" ::"v"(ra[u]));
        asm volatile("" ::"v"(rb[u]));
    }
    // ---- the last tile's stream: nothing left to multiply.  What the last k loop left in the slots (landed), then the parked
    // tile's row groups four at a time -- twelve loads in flight per wave (everything asm has drained: hipcc schedules this) ----
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        opt_pin(sl[k]);
        opt_update_store(sl[k]);
    }
    dr_wait<0>();
#if !(GD_ADAMW_DBG & 32)  // (probe bit 5: the last tile's row groups are not updated -- prices this drain; results wrong)
    {
        const DrAdamProd& g = d.p[pp];
        const int c_bytes = (int)c_bytes_of(pp);
        const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(g.W, 0, c_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rM = __builtin_amdgcn_make_buffer_rsrc(g.ea, 0, c_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(g.ea2, 0, c_bytes, 0x00020000);
        for (; pend_g < 16; pend_g += 4) {
            f32x4 pv[4], mv[4], vv[4];
            uint32_t oo[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                oo[u] = (pend_lane && !(GD_ADAMW_DBG & 2)) ? pend_base + (uint32_t)(pend_g + u) * ldc4 : PARK;
                pv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rW, oo[u], 0, 0));
                mv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rM, oo[u], 0, 0));
                vv[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rV, oo[u], 0, 0));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int gi = pend_g + u;
                const float* sg = reinterpret_cast<const float*>(stash + 256 * (gi & 3)) + (gi >> 2);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float pk = pv[u][k], mk = mv[u][k], vk = vv[u][k];
                    gd_adam_elem(pk, sg[256 * k], mk, vk, hy);
                    pv[u][k] = pk;
                    mv[u][k] = mk;
                    vv[u][k] = vk;
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pv[u]), rW, oo[u], 0, 2);  // (aux 2 = nt)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, mv[u]), rM, oo[u], 0, 2);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, vv[u]), rV, oo[u], 0, 2);
            }
        }
    }
#endif
}

template <int D, bool NTL>
int dr_tn_adamw_go(const DrMultiArgs& d, hipStream_t s) {
    static bool attr_set = false;  // 8 waves x 16 KB: the tile whose optimiser stream is running
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dr_tn_adamw_kernel<D, NTL>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (e != hipSuccess) {
            gdmcf_set_error("hipFuncSetAttribute(dr_tn_adamw_kernel, LDS=128 KB): %s", hipGetErrorString(e));
            return GDMCF_E_HIP;
        }
        attr_set = true;
    }
    hipLaunchKernelGGL((dr_tn_adamw_kernel<D, NTL>), dim3(dr_cu_count()), dim3(512), 128 * 1024, s, d);
    return GDMCF_OK;
}

template <int D>
int dr_tn_adamw_go(const DrMultiArgs& d, hipStream_t s) {
    // rows of W / exp_avg / exp_avg_sq on 128-byte lines in every product: the stream's loads need not stay in L2 (dr_load0_rw)
    bool lines = true;
    for (int i = 0; i < d.n; ++i) {
        const DrAdamProd& p = d.p[i];
        lines = lines && (p.ldc & 31) == 0 && (((uintptr_t)p.W | (uintptr_t)p.ea | (uintptr_t)p.ea2) & 127) == 0;
    }
    static const int force = gd_env_int("GDMCF_DR_NT_LOADS", -1);  // tuning knob: 0 / 1
    return (force >= 0 ? force != 0 : lines) ? dr_tn_adamw_go<D, true>(d, s) : dr_tn_adamw_go<D, false>(d, s);
}

template <int D>
int dr_tn_go(const DrArgs& d, hipStream_t s) {
    hipLaunchKernelGGL((dr_tn_kernel<1, 1, D>), dim3(dr_cu_count()), dim3(512), 0, s, d);
    return GDMCF_OK;
}

}  // namespace

// Ticket-counter set of one launch.  Two launches that overlap in time -- the two weight gradients of a step on two streams
// (GDMCF_GEMM_SIDE=1), two host threads, a replayed graph beside an eager step -- must not draw from the same counters, or each
// computes only a subset of its tiles.  The set therefore belongs to the LAUNCH, not to the call site: eager launches rotate
// through sets 0..15, launches recorded during a stream capture through 16..31 (a graph node keeps its set for every replay, so
// it must never meet an eager launch's).  Limits that follow: at most 16 eager launches of these kernels in flight at once, and
// at most 16 captured ones among all graphs that replay concurrently -- stream order and graph order serialise far below that.
static std::atomic<unsigned> g_dr_seq_eager{0}, g_dr_seq_graph{0};
static int dr_ticket_slot(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();  // (the legacy stream while another stream captures: not a capture of this launch)
        st = hipStreamCaptureStatusNone;
    }
    if (st == hipStreamCaptureStatusActive) return 16 + (int)(g_dr_seq_graph.fetch_add(1, std::memory_order_relaxed) & 15u);
    return (int)(g_dr_seq_eager.fetch_add(1, std::memory_order_relaxed) & 15u);
}

// Tiles, ticket order and k-steps of a weight-gradient product on the register-streaming kernels (dr_tn_kernel /
// dr_tn_adamw_kernel); false when they do not take it.  With a bias-column request (operand B one column wider than the product:
// linear.hip) g.N counts that column on return and *bias_db is the vector it goes to, else NULL; *depth is the ring depth D.
static bool dr_tn_prepare(int epi, GdGemm& g, DrArgs& d, float** bias_db, int* depth) {
    const int64_t lim = (int64_t)1 << 32;  // 32-bit byte offsets inside every matrix
    if ((int64_t)g.K * g.lda * 4 >= lim || (int64_t)g.K * g.ldb * 4 >= lim || (int64_t)g.M * g.ldc * 4 >= lim) return false;
    if (g.lda < g.M || g.ldb < g.N || g.ldc < g.N) return false;
    const long tiles = (long)gd_cdiv(g.M, 64) * gd_cdiv(g.N, 64);
    if (tiles < 512 || g.K < 128) return false;  // (short reductions: a tile is all prologue; the LDS-tiled kernels take them)
    // bias gradient requested as one more column of the product (linear.hip: operand B carries the row scale in column N): the
    // kernel multiplies N + 1 columns -- the extra one needs its lane's 4-column group to straddle the end, i.e. N % 4 == 0 or
    // any N (the straddle path stores element-wise) -- and writes it to out2 instead of C
    *bias_db = (g.ldb > g.N) ? g.out2 : nullptr;
    if (*bias_db) g.N += 1;
    d.tiles_m = gd_cdiv(g.M, 64);
    d.tiles_n = gd_cdiv(g.N, 64);
    d.m_fastest = d.tiles_m <= d.tiles_n;  // tiles that share the LARGER operand's panel draw consecutive tickets
    {   // tuning knob: GDMCF_DR_MF=0|1 forces the ticket order of the fused-AdamW product
        static const int mf = gd_env_int("GDMCF_DR_MF", -1);
        if (mf >= 0 && epi == GD_EPI_ADAMW) d.m_fastest = mf;
    }
    const int ks = gd_cdiv(g.K, 4);
    // ring depth: the one whose size wastes the fewest padded steps per tile
    int best = 9, waste = 1 << 30;
    for (int dd : {9, 8, 7}) {
        const int w = gd_cdiv(ks, dd + 1) * (dd + 1) - ks;
        if (w < waste) { waste = w; best = dd; }
    }
    {   // tuning knob: GDMCF_DR_D=7|8|9 forces the ring depth
        static const int forced = gd_env_int("GDMCF_DR_D", 0);
        if (forced >= 7 && forced <= 9) { best = forced; waste = gd_cdiv(ks, best + 1) * (best + 1) - ks; }
    }
    d.ksp = ks + waste;
    *depth = best;
    g.tiles_m = d.tiles_m;
    g.tiles_n = d.tiles_n;
    return true;
}

static DrAdamProd dr_adam_prod(const GdGemm& g, const DrArgs& d, float* bias_db) {
    DrAdamProd p = {};
    p.A = g.A; p.B = g.B; p.W = g.C; p.ea = const_cast<float*>(g.aux); p.ea2 = const_cast<float*>(g.aux2); p.bias = bias_db;
    p.lda = (int)g.lda; p.ldb = (int)g.ldb; p.ldc = (int)g.ldc;
    p.M = g.M; p.N = g.N; p.K = g.K;
    p.tiles_m = d.tiles_m; p.tiles_n = d.tiles_n; p.m_fastest = d.m_fastest;
    p.adam = g.adam;
    p.adam_dev = g.adam_dev;  // a bound graph step state (linear.hip)
    return p;
}

static int dr_adamw_launch(DrMultiArgs& m, int depth, hipStream_t s) {
    m.ctr = dr_ticket_slot(s);
    if (depth == 9) return dr_tn_adamw_go<9>(m, s);
    if (depth == 8) return dr_tn_adamw_go<8>(m, s);
    return dr_tn_adamw_go<7>(m, s);
}

// (the fused-AdamW epilogue: hipcc rotates accumulators through ring slots there, which the first, set-based lint
// (build.py:lint_ring_registers) cannot tell from a copy of in-flight data; the per-register analysis that replaced it for
// this variant (lint_vmcnt: no instruction touches a register whose load the counted waits do not cover) verifies it clean,
// and tests/test_gpu_fullsize.py checks every element of W / exp_avg / exp_avg_sq at the full shapes.  GDMCF_DR_ADAMW=0 sends
// the fused products back to the LDS-tiled kernel.)
static bool dr_fused_on() { return dr_routes().dw && dr_routes().adamw; }

// Several weight-gradient products with AdamW as ONE launch of dr_tn_adamw_kernel (gdmcf_linear_bwd_weight_adamw_multi_f32).
// All or nothing: GD_DR_NOT_TAKEN (nothing launched) unless every product is one the kernel takes, in f32, with the same ring
// depth and k-steps per tile.  A product whose bias column was taken has its out2 cleared, as gd_dr_tn_launch does.
int gd_gemm_dr_adamw_multi(GdGemm* gs, int n, hipStream_t s) {
    if (n < 1 || n > DR_MULTI_MAX || !dr_fused_on()) return GD_DR_NOT_TAKEN;
    DrMultiArgs m = {};
    float* bias_db[DR_MULTI_MAX] = {};
    int n_user[DR_MULTI_MAX] = {};
    int depth = 0;
    bool ok = true;
    double flop = 0.0;
    for (int i = 0; i < n && ok; ++i) {
        GdGemm& g = gs[i];
        ok = !g.bf16 && !g.accumulate && !g.C16 && g.splits <= 1;
        DrArgs d = {};
        int dep = 0;
        n_user[i] = g.N;
        if (ok) ok = dr_tn_prepare(GD_EPI_ADAMW, g, d, &bias_db[i], &dep);
        if (ok) {
            ok = (i == 0 || (dep == depth && d.ksp == m.ksp)) && (long)d.tiles_m * d.tiles_n < (1L << DR_VT_SHIFT);
            depth = dep;
            m.ksp = d.ksp;
            m.p[i] = dr_adam_prod(g, d, bias_db[i]);
            flop += 2.0 * g.M * n_user[i] * g.K;
        }
    }
    if (!ok) {
        for (int i = 0; i < n; ++i) gs[i].N = n_user[i] ? n_user[i] : gs[i].N;
        return GD_DR_NOT_TAKEN;
    }
    m.n = n;
    m.stagger = dr_stagger();
    {
        GdProfScope prof(gs[0].prof_tag, flop, s);
        const int rc = dr_adamw_launch(m, depth, s);
        if (rc != GDMCF_OK) return rc;
    }
    for (int i = 0; i < n; ++i) {
        gs[i].N = n_user[i];
        if (bias_db[i]) gs[i].out2 = nullptr;  // taken: the caller skips its column-sum pass
    }
    t_gd_last_gemm = 3;
    return gd_launch_status("gemm_dr");
}

// The plain weight gradient on dr_tn_kernel, or GD_DR_NOT_TAKEN with g as it was.
int gd_dr_tn_launch(GdGemm& g, hipStream_t s) {
    if (!dr_routes().dw) return GD_DR_NOT_TAKEN;
    DrArgs d = {};
    d.stagger = dr_stagger();
    const int n_user = g.N;
    float* bias_db = nullptr;
    int best = 9;
    if (!dr_tn_prepare(GD_EPI_STORE, g, d, &bias_db, &best)) {
        g.N = n_user;
        return GD_DR_NOT_TAKEN;
    }
    d.g = g;
    d.ctr = dr_ticket_slot(s);
    d.g.out2 = bias_db;
    {
        GdProfScope prof(g.prof_tag, 2.0 * g.M * n_user * g.K, s);
        int rc_ = best == 9 ? dr_tn_go<9>(d, s) : best == 8 ? dr_tn_go<8>(d, s) : dr_tn_go<7>(d, s);
        if (rc_ != GDMCF_OK) return rc_;
    }
    g.N = n_user;
    t_gd_last_gemm = 2;
    if (bias_db) g.out2 = nullptr;  // taken: the caller skips its column-sum pass
    return gd_launch_status("gemm_dr");
}

// gdmcf_debug_dr_tn_plan (include/gdmcf_hip.h): dr_tn_prepare on a scratch product, nothing launched.  Shapes as the weight-
// gradient entries name them (batch M, dW[N, K]); the product is built as linear.hip builds it in float32 mode.
extern "C" int gdmcf_debug_dr_tn_plan(int M, int N, int K, int64_t lddz, int64_t lda, int64_t ldw, int bias_col, int fused,
                                      int* depth, int* ksp, int* tiles_m, int* tiles_n, int* m_fastest, int* has_bias) {
    static float db_scratch;  // (never written: only its address travels, as the bias gradient's would)
    GdGemm g = {};
    DrArgs d = {};
    float* bias_db = nullptr;
    int dep = 0;
    bool ok = M > 0 && N > 0 && K > 0 && lddz >= N && lda >= K && ldw >= K && (fused ? dr_fused_on() : dr_routes().dw);
    if (ok) {
        g.lda = lddz; g.ldb = lda; g.ldc = ldw; g.M = N; g.N = K; g.K = M; g.splits = 1;
        g.out2 = (bias_col && lda > K) ? &db_scratch : nullptr;  // (linear.hip: bias_col_request)
        ok = dr_tn_prepare(fused ? GD_EPI_ADAMW : GD_EPI_STORE, g, d, &bias_db, &dep);
        if (ok && fused) ok = (long)d.tiles_m * d.tiles_n < (1L << DR_VT_SHIFT);
    }
    if (depth) *depth = ok ? dep : 0;
    if (ksp) *ksp = ok ? d.ksp : 0;
    if (tiles_m) *tiles_m = ok ? d.tiles_m : 0;
    if (tiles_n) *tiles_n = ok ? d.tiles_n : 0;
    if (m_fastest) *m_fastest = ok ? d.m_fastest : 0;
    if (has_bias) *has_bias = ok && bias_db != nullptr;
    return ok ? 1 : 0;
}
