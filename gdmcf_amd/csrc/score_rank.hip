// gdmcf_score_rank_f32: the exact catalogue ranks of named items (held-out targets) from the fused score product -- score_topk.hip's
// product with its selection stage replaced by the counting rank.hip does on stored rows.  The [n_rows, n_items] score matrix
// exists only as MFMA accumulators; the order is rank_order.h's, the conventions are gdmcf_rank_targets_f32's.
//
// Three launches:
//   1. score_rank_targets_kernel -- one wave per (row, 16 of its targets): the user row in every A row, the 16 target item rows in
//      B, the product step of score_product.h, so a target's score carries the bits the stream forms for that item (a rank counts
//      the pairs STRICTLY above the target's own: another summation order would let a target count itself).  The wave scans the
//      row's mask entries for its targets and writes the 64-bit (key, ~index) pairs to the workspace; pair 0 = no target there.
//   2. score_rank_kernel -- workgroups of (row tile, item slab) laid out as score_topk_kernel's.  Per pass of GP targets: the
//      tile's pairs sorted descending per row in LDS, one counter per gap; the slab is streamed (next step's items requested before
//      this step's MFMAs, mask bitmap rebuilt per 2048-item window); each of a lane's 4 RB scores is located among its row's
//      targets by binary search (branch-free, four rows side by side) and the gap counter bumped (LDS integer atomic).  Scores
//      below the row's lowest target are counted in a register and skip bitmap, search and atomic.  The gap counts go to the
//      workspace as one row per slab.
//   3. score_rank_finish_kernel -- sorts the pairs again, adds the slabs' counts, takes the prefix sum and writes every target
//      column's rank; n_live from the bitmap windows' population counts, summed the same way.
// Integer sums only: the result is the same bits in every run whatever order waves and slabs arrive in.
#include "common.h"
#include "rank_order.h"
#include "score_product.h"

namespace {

typedef unsigned long long u64;
constexpr int SR_BM_ITEMS = 2048;  // items covered by one build of the history bitmap
constexpr int SR_BM_WORDS = SR_BM_ITEMS / 32;

__device__ __forceinline__ u64 sr_pair(uint32_t key, int i) { return ((u64)key << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i); }

// ---- 1. the targets' own pairs -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_rank_targets_kernel(const float* __restrict__ U, int64_t ldu, const int64_t* __restrict__ uid,
                                                                  int n_rows, const float* __restrict__ V, int64_t ldi, int n_items, int d,
                                                                  const int64_t* __restrict__ mptr, const int32_t* __restrict__ midx,
                                                                  const int64_t* __restrict__ tptr, const int32_t* __restrict__ tidx, int G,
                                                                  int Gpad, int vec, u64* __restrict__ pairs) {
    const int lane = threadIdx.x & 63, lc = lane & 15, lg = lane >> 4;
    const int groups = Gpad >> 4;
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= (int64_t)n_rows * groups) return;  // (wave-uniform; no barrier in this kernel)
    const int row = (int)(gw / groups), grp = (int)(gw - (int64_t)row * groups);
    const int64_t tbeg = tptr[row];
    const int64_t tlen = tptr[row + 1] - tbeg;
    const int len = (int)(tlen < (int64_t)G ? (tlen > 0 ? tlen : 0) : (int64_t)G);
    const int col = grp * 16 + lc;
    const int t = col < len ? tidx[tbeg + col] : -1;
    const bool valid = t >= 0 && t < n_items;
    if (grp * 16 >= len) {  // nothing named in these 16 columns
        if (lg == 0) pairs[(int64_t)row * Gpad + col] = 0ull;
        return;
    }
    // score(row, t) for the 16 targets: every A row is the user row, B row lc is item t (item 0 stands in where there is none)
    const float* arow[1] = {U + (uid ? uid[row] : (int64_t)row) * ldu};
    const float* brow = V + (int64_t)(valid ? t : 0) * ldi;
    f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
    sp_mfma_reread<1>(acc, arow, brow, lg, d, vec != 0);
    const float score = acc[0][0];  // (row 4 lg of the 16 equal rows, column lc)
    // which of the 16 targets does the row's mask name?
    uint32_t hit = 0u;
    if (mptr) {
        int tv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) tv[i] = __shfl(valid ? t : -1, i);
        const int64_t beg = mptr[row], end = mptr[row + 1];
        for (int64_t j = beg + lane; j < end; j += 64) {
            const int c = midx[j];
            if (c >= 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) hit |= (c == tv[i]) ? (1u << i) : 0u;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) hit |= __shfl_xor(hit, o);
    }
    if (lg == 0) {
        u64 p = 0ull;
        if (valid) p = sr_pair((hit >> lc) & 1u ? NEG_INF_KEY : order_key(score), t);
        pairs[(int64_t)row * Gpad + col] = p;
    }
}

// ---- shared by the main and the finish launch: pass `base` of the tile's pairs into LDS, sorted descending per row ----------
// sorted [R][GP] (GP a power of two): the pairs of columns base .. base + GP - 1 of rows row0 .. row0 + rows_here - 1, 0 elsewhere
// (below every real pair: they sink to the end); nv[r] = the row's real pairs of this pass.  Ends with a barrier.
__device__ void sr_sorted_pass(u64* sorted, uint32_t* nv, const u64* __restrict__ pairs, int row0, int rows_here, int R, int GP,
                               int base, int Gpad, int tid) {
    for (int e = tid; e < R * GP; e += 256) {
        const int r = e / GP, j = e - r * GP;
        sorted[e] = (r < rows_here && base + j < Gpad) ? pairs[(int64_t)(row0 + r) * Gpad + base + j] : 0ull;
    }
    __syncthreads();
    const int half = GP >> 1;
    for (int size = 2; size <= GP; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = tid; e < R * half; e += 256) {
                const int r = e / half, j = e - r * half;
                const int lo = ((j / stride) * stride * 2) + (j % stride);
                const int hi = lo + stride;
                const bool desc = ((lo & size) == 0);
                u64* c = sorted + (size_t)r * GP;
                const u64 a = c[lo], b = c[hi];
                if ((a < b) == desc) {
                    c[lo] = b;
                    c[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int r = tid; r < R; r += 256) {
        const u64* c = sorted + (size_t)r * GP;
        int lo = 0, hi = GP;  // the entries ahead of the first pair 0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] != 0ull) lo = mid + 1;
            else hi = mid;
        }
        nv[r] = (uint32_t)lo;
    }
    __syncthreads();
}

struct SrArgs {
    const float* U;
    int64_t ldu;
    const int64_t* uid;
    int n_rows;
    const float* V;
    int64_t ldi;
    int n_items, d;
    const int64_t* mptr;
    const int32_t* midx;
    int R, GP, npass, Gpad, nslab, slab_items, vec;
    const u64* pairs;     // [n_rows][Gpad]
    uint32_t* slab_cnt;   // [n_rows][npass][nslab][GP + 1]
    uint32_t* slab_mask;  // [n_rows][nslab]: distinct in-range mask entries of the row inside the slab
};

// ---- 2. the stream -----------------------------------------------------------------------------------------------------------
template <int RB, bool AREG>
__global__ __launch_bounds__(256) void score_rank_kernel(const SrArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int R = g.R, GP = g.GP;
    u64* sorted = reinterpret_cast<u64*>(smem_raw);                        // [R][GP]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(sorted + (size_t)R * GP);  // [R][GP + 1]
    uint32_t* nv = cnt + (size_t)R * (GP + 1);                             // [R]
    uint32_t* nmask = nv + R;                                              // [R]
    uint32_t* bitmap = nmask + R;                                          // [R][SR_BM_WORDS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x / g.nslab, slab = blockIdx.x - tile * g.nslab;
    const int row0 = tile * R;
    const int rows_here = min(R, g.n_rows - row0);
    const int n_items = g.n_items, d = g.d;
    const int i0 = slab * g.slab_items, i1 = min(n_items, i0 + g.slab_items);
    const int lc = lane & 15, lg = lane >> 4;
    const bool vec = g.vec != 0;

    for (int r = tid; r < R; r += 256) nmask[r] = 0u;
    // the tile's rows of the user table (rows past the end repeat the last one and are never counted for)
    const float* arow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = row0 + min(rb * 16 + lc, rows_here - 1);
        arow[rb] = g.U + (g.uid ? g.uid[r] : (int64_t)r) * g.ldu;
    }
    f32x4 areg[RB][4];
    if constexpr (AREG) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) sp_load_frags(areg[rb], arow[rb], lg, d, vec);
    }
    auto item_row = [&](int base) -> const float* { return g.V + (int64_t)min(base + 16 * wave + lc, n_items - 1) * g.ldi; };

    for (int pass = 0; pass < g.npass; ++pass) {
        __syncthreads();  // (the previous pass's counters have been written out)
        sr_sorted_pass(sorted, nv, g.pairs, row0, rows_here, R, GP, pass * GP, g.Gpad, tid);
        for (int e = tid; e < R * (GP + 1); e += 256) cnt[e] = 0u;
        // this lane's rows: the float of the lowest target's key.  x < lowf (neither a NaN) puts x's key strictly below that key,
        // and a mask can only lower the key of such an x: the pair is below every target whatever the bitmap says.  Rows without
        // targets (and rows past the end) take +inf: (nearly) everything is skipped, and nothing is ever searched for them.
        float lowf[RB][4];
        uint32_t below[RB][4];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = rb * 16 + 4 * lg + q;
                const int n = (int)nv[r];
                lowf[rb][q] = n > 0 ? key_to_float((uint32_t)(sorted[(size_t)r * GP + n - 1] >> 32)) : INFINITY;
                below[rb][q] = 0u;
            }
        f32x4 bcur[4], bnext[4];
        if constexpr (AREG) sp_load_frags(bcur, item_row(i0), lg, d, vec);

        for (int cbase = i0; cbase < i1; cbase += SR_BM_ITEMS) {
            const int cend = min(i1, cbase + SR_BM_ITEMS);
            // ---- history bitmap of items cbase .. cend - 1 ----
            __syncthreads();
            for (int e = tid; e < R * SR_BM_WORDS; e += 256) bitmap[e] = 0u;
            __syncthreads();
            if (g.mptr) {
                for (int r = wave; r < rows_here; r += 4) {
                    const int64_t beg = g.mptr[row0 + r], end = g.mptr[row0 + r + 1];
                    for (int64_t j = beg + lane; j < end; j += 64) {
                        const int m = g.midx[j];
                        if (m >= cbase && m < cend) atomicOr(&bitmap[r * SR_BM_WORDS + ((m - cbase) >> 5)], 1u << ((m - cbase) & 31));
                    }
                }
            }
            __syncthreads();
            if (pass == 0 && g.mptr) {  // the window's masked items (row r belongs to wave r & 3 alone)
                for (int r = wave; r < rows_here; r += 4) {
                    uint32_t pc = (uint32_t)__popc(bitmap[r * SR_BM_WORDS + lane]);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) pc += __shfl_xor(pc, o);
                    if (lane == 0) nmask[r] += pc;
                }
            }
            for (int base = cbase; base < cend; base += SP_STEP) {
                f32x4 acc[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (AREG) {
                    // the next step's items are requested before this step's products (addresses clamped to the table)
                    sp_load_frags(bnext, item_row(base + SP_STEP), lg, d, vec);
                    sp_mfma_frags<RB>(acc, areg, bcur, d);
#pragma unroll
                    for (int j = 0; j < 4; ++j) bcur[j] = bnext[j];
                } else {
                    sp_mfma_reread<RB>(acc, arow, item_row(base), lg, d, vec);
                }
                // ---- counting: acc[rb][q] = score(row rb*16 + 4*lg + q, item base + 16*wave + lc) ----
                const int item = base + 16 * wave + lc;
                if (item < i1) {
                    const int bi = item - cbase;
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        // four rows at a time: their searches run side by side, branch-free, so the LDS reads of one hide behind
                        // the others'.  The padded list has GP = 2^k entries, the pairs 0 at its end are below every p: the count of
                        // entries >= p over the whole list is the count over the row's nv targets
                        bool act[4];
                        bool any = false;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            act[q] = !(acc[rb][q] < lowf[rb][q]);
                            below[rb][q] += act[q] ? 0u : 1u;
                            any = any || act[q];
                        }
                        if (!any) continue;
                        const int r0 = rb * 16 + 4 * lg;
                        const uint32_t inwin = 1u << (bi & 31);
                        u64 p[4];
                        int lo[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            uint32_t key = order_key(acc[rb][q]);
                            if (bitmap[(r0 + q) * SR_BM_WORDS + (bi >> 5)] & inwin) key = NEG_INF_KEY;
                            p[q] = sr_pair(key, item);
                            lo[q] = 0;
                        }
                        const u64* c0 = sorted + (size_t)r0 * GP;
                        for (int st = GP >> 1; st > 0; st >>= 1) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) lo[q] += (c0[q * GP + lo[q] + st - 1] >= p[q]) ? st : 0;
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) lo[q] += (c0[q * GP + lo[q]] >= p[q]) ? 1 : 0;  // (all GP entries at or above p)
                        // (a row without targets counts into its gap 0, which nothing reads)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (act[q]) atomicAdd(&cnt[(size_t)(r0 + q) * (GP + 1) + lo[q]], 1u);
                    }
                }
            }
        }
        // the skipped scores sit below every target of their row: gap nv.  (16 lanes share a row: added up first)
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t b = below[rb][q];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) b += __shfl_xor(b, o);
                const int r = rb * 16 + 4 * lg + q;
                if (lc == 0 && b && r < rows_here) atomicAdd(&cnt[(size_t)r * (GP + 1) + nv[r]], b);
            }
        __syncthreads();
        for (int e = tid; e < rows_here * (GP + 1); e += 256) {
            const int r = e / (GP + 1), j = e - r * (GP + 1);
            g.slab_cnt[(((int64_t)(row0 + r) * g.npass + pass) * g.nslab + slab) * (GP + 1) + j] = cnt[e];
        }
    }
    __syncthreads();
    for (int r = tid; r < rows_here; r += 256) g.slab_mask[(int64_t)(row0 + r) * g.nslab + slab] = nmask[r];
}

// ---- 3. slabs added, prefix sum, the ranks ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_rank_finish_kernel(const SrArgs g, int G, int32_t* __restrict__ rank_out, int64_t ldr,
                                                                 int32_t* __restrict__ n_live_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int R = g.R, GP = g.GP;
    u64* sorted = reinterpret_cast<u64*>(smem_raw);                        // [R][GP]
    uint32_t* cnt = reinterpret_cast<uint32_t*>(sorted + (size_t)R * GP);  // [R][GP + 1]
    uint32_t* nv = cnt + (size_t)R * (GP + 1);                             // [R]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * R;
    const int rows_here = min(R, g.n_rows - row0);
    if (n_live_out) {
        for (int r = tid; r < rows_here; r += 256) {
            uint32_t m = 0;
            for (int s = 0; s < g.nslab; ++s) m += g.slab_mask[(int64_t)(row0 + r) * g.nslab + s];
            n_live_out[row0 + r] = g.n_items - (int)m;
        }
    }
    for (int pass = 0; pass < g.npass; ++pass) {
        const int base = pass * GP;
        __syncthreads();
        sr_sorted_pass(sorted, nv, g.pairs, row0, rows_here, R, GP, base, g.Gpad, tid);
        for (int e = tid; e < rows_here * (GP + 1); e += 256) {
            const int r = e / (GP + 1), j = e - r * (GP + 1);
            const uint32_t* p = g.slab_cnt + (((int64_t)(row0 + r) * g.npass + pass) * g.nslab) * (GP + 1) + j;
            uint32_t v = 0;
            for (int s = 0; s < g.nslab; ++s) v += p[(int64_t)s * (GP + 1)];
            cnt[e] = v;
        }
        __syncthreads();
        // inclusive prefix sum of every row's counters: entry m = items strictly above the target sorted to place m
        for (int r = wave; r < rows_here; r += 4) {
            uint32_t* c = cnt + (size_t)r * (GP + 1);
            uint32_t carry = 0;
            for (int c0 = 0; c0 < GP; c0 += 64) {
                uint32_t v = c0 + lane < GP ? c[c0 + lane] : 0u;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t t = __shfl_up(v, o);
                    if (lane >= o) v += t;
                }
                v += carry;
                if (c0 + lane < GP) c[c0 + lane] = v;
                carry = __shfl(v, 63);
            }
        }
        __syncthreads();
        const int ncol = min(GP, G - base);  // the columns of this pass
        for (int e = tid; e < rows_here * ncol; e += 256) {
            const int r = e / ncol, j = e - r * ncol;
            const u64 p = g.pairs[(int64_t)(row0 + r) * g.Gpad + base + j];
            int32_t rank = -1;
            if (p != 0ull) {
                const u64* c = sorted + (size_t)r * GP;
                int lo = 0, hi = (int)nv[r];  // number of targets strictly above p: the first entry that equals p
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (c[mid] > p) lo = mid + 1;
                    else hi = mid;
                }
                rank = (int32_t)cnt[(size_t)r * (GP + 1) + lo];
            }
            rank_out[(int64_t)(row0 + r) * ldr + base + j] = rank;
        }
    }
}

struct SrPlan {
    int RB, R, GP, npass, Gpad, nslab, slab_items;
    size_t off_cnt, off_mask, bytes;
};

// Tile height and targets per pass by G -- 12 bytes of LDS per (row, target of a pass): 64 rows to G = 128, 32 to 256, 16 above,
// 512 targets a pass (96 KiB each, beside the R x 64-word bitmap window and 4 (3 R) bytes of control words) -- and the item slabs as
// st_plan cuts them: enough workgroups for two per CU, slabs of whole steps of at least 512 items, slab counts of at most 5 % of the
// score matrix they stand in for.
SrPlan sr_plan(int n_rows, int n_items, int G) {
    SrPlan p;
    if (G <= 128) { p.RB = 4; p.R = 64; }
    else if (G <= 256) { p.RB = 2; p.R = 32; }
    else { p.RB = 1; p.R = 16; }
    p.GP = 16;
    while (p.GP < G && p.GP < 512) p.GP <<= 1;
    p.npass = gd_cdiv(G, p.GP);
    p.Gpad = gd_cdiv(G, 16) * 16;
    const int tiles = gd_cdiv(n_rows, p.R);
    int want = tiles >= 256 ? 1 : gd_cdiv(512, tiles);
    const int64_t by_ws = (int64_t)n_items / (20 * (int64_t)(p.GP + 1));
    const int64_t by_len = (int64_t)n_items / 512;
    if (want > 16) want = 16;
    if (want > by_ws) want = (int)by_ws;
    if (want > by_len) want = (int)by_len;
    if (want < 1) want = 1;
    p.slab_items = gd_cdiv(gd_cdiv(n_items, want), SP_STEP) * SP_STEP;
    p.nslab = gd_cdiv(n_items, p.slab_items);
    p.off_cnt = (size_t)n_rows * p.Gpad * sizeof(u64);
    p.off_mask = p.off_cnt + (size_t)n_rows * p.npass * p.nslab * (p.GP + 1) * sizeof(uint32_t);
    p.bytes = p.off_mask + (size_t)n_rows * p.nslab * sizeof(uint32_t);
    return p;
}

size_t sr_lds(const SrPlan& p) {
    return (size_t)p.R * p.GP * 8 + (size_t)p.R * (p.GP + 1) * 4 + (size_t)p.R * 2 * 4 + (size_t)p.R * SR_BM_WORDS * 4;
}

}  // namespace

extern "C" {

int gdmcf_debug_score_rank_plan(int n_rows, int n_items, int G, int* tile_rows, int* pass_targets, int* passes, int* slabs) {
    if (n_rows <= 0 || n_items <= 0 || G < 1) {
        if (tile_rows) *tile_rows = 0;
        if (pass_targets) *pass_targets = 0;
        if (passes) *passes = 0;
        if (slabs) *slabs = 0;
        return 0;
    }
    const SrPlan p = sr_plan(n_rows, n_items, G);
    if (tile_rows) *tile_rows = p.R;
    if (pass_targets) *pass_targets = p.GP;
    if (passes) *passes = p.npass;
    if (slabs) *slabs = p.nslab;
    return 1;
}

size_t gdmcf_score_rank_ws_bytes(int n_rows, int n_items, int d, int G) {
    (void)d;
    if (n_rows <= 0 || n_items <= 0 || G < 1) return 0;
    return sr_plan(n_rows, n_items, G).bytes;
}

int gdmcf_score_rank_f32(const float* user_emb, int64_t ldu, const int64_t* user_ids, int n_rows, const float* item_emb, int64_t ldi,
                         int n_items, int d, const int64_t* mask_indptr, const int32_t* mask_indices, const int64_t* tgt_indptr,
                         const int32_t* tgt_indices, int G, int32_t* rank_out, int64_t ldr, int32_t* n_live_out, void* ws,
                         size_t ws_bytes, void* stream) {
    GD_CHECK_SHAPE(n_rows > 0 && n_items > 0 && d >= 1 && ldu >= d && ldi >= d, "gdmcf_score_rank_f32: bad shape");
    GD_CHECK_SHAPE(G >= 1 && ldr >= G, "gdmcf_score_rank_f32: bad shape (G >= 1, ldr >= G)");
    GD_CHECK_ARG(d <= 4096, "gdmcf_score_rank_f32: d > 4096 unsupported");
    GD_CHECK_ARG(user_emb && item_emb && rank_out && tgt_indptr && tgt_indices,
                 "gdmcf_score_rank_f32: null user_emb / item_emb / rank_out / targets");
    GD_CHECK_ARG((mask_indptr == nullptr) == (mask_indices == nullptr), "gdmcf_score_rank_f32: mask indptr/indices mismatch");
    const SrPlan p = sr_plan(n_rows, n_items, G);
    if (ws == nullptr || ws_bytes < p.bytes) {
        gdmcf_set_error("gdmcf_score_rank_f32: workspace of %zu B, %zu needed (gdmcf_score_rank_ws_bytes)", ws ? ws_bytes : (size_t)0,
                        p.bytes);
        return GDMCF_E_WORKSPACE;
    }
    GD_CHECK_ARG(gd_aligned16(ws), "gdmcf_score_rank_f32: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int vec = (d % 4 == 0) && (ldu % 4 == 0) && (ldi % 4 == 0) && gd_aligned16(user_emb) && gd_aligned16(item_emb);
    const size_t lds = sr_lds(p);
    const bool areg = d <= 64;
    static bool attr_set = false;
    if (!attr_set) {
        const void* fns[7] = {reinterpret_cast<const void*>(&score_rank_kernel<4, true>), reinterpret_cast<const void*>(&score_rank_kernel<4, false>),
                              reinterpret_cast<const void*>(&score_rank_kernel<2, true>), reinterpret_cast<const void*>(&score_rank_kernel<2, false>),
                              reinterpret_cast<const void*>(&score_rank_kernel<1, true>), reinterpret_cast<const void*>(&score_rank_kernel<1, false>),
                              reinterpret_cast<const void*>(&score_rank_finish_kernel)};
        bool ok = true;
        for (int i = 0; i < 7; ++i) ok = ok && hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        if (!ok) {
            gdmcf_set_error("gdmcf_score_rank_f32: hipFuncSetAttribute failed");
            return GDMCF_E_HIP;
        }
        attr_set = true;
    }
    unsigned char* wsb = reinterpret_cast<unsigned char*>(ws);
    u64* pairs = reinterpret_cast<u64*>(wsb);
    SrArgs g = {user_emb, ldu, user_ids, n_rows, item_emb, ldi, n_items, d, mask_indptr, mask_indices, p.R, p.GP, p.npass, p.Gpad, p.nslab,
                p.slab_items, vec, pairs, reinterpret_cast<uint32_t*>(wsb + p.off_cnt), reinterpret_cast<uint32_t*>(wsb + p.off_mask)};
    const int tiles = gd_cdiv(n_rows, p.R);
    const int64_t twaves = (int64_t)n_rows * (p.Gpad / 16);
    {
        GdProfScope prof(12, 2.0 * n_rows * (double)n_items * d * p.npass, s);  // (all three launches)
        hipLaunchKernelGGL(score_rank_targets_kernel, dim3((unsigned)((twaves + 3) / 4)), dim3(256), 0, s, user_emb, ldu, user_ids, n_rows,
                           item_emb, ldi, n_items, d, mask_indptr, mask_indices, tgt_indptr, tgt_indices, G, p.Gpad, vec, pairs);
        const dim3 grid((unsigned)tiles * (unsigned)p.nslab);
#define GD_SR_LAUNCH(RB_, AR_) hipLaunchKernelGGL((score_rank_kernel<RB_, AR_>), grid, dim3(256), lds, s, g)
        if (p.RB == 4 && areg) GD_SR_LAUNCH(4, true);
        else if (p.RB == 4) GD_SR_LAUNCH(4, false);
        else if (p.RB == 2 && areg) GD_SR_LAUNCH(2, true);
        else if (p.RB == 2) GD_SR_LAUNCH(2, false);
        else if (areg) GD_SR_LAUNCH(1, true);
        else GD_SR_LAUNCH(1, false);
#undef GD_SR_LAUNCH
        hipLaunchKernelGGL(score_rank_finish_kernel, dim3(tiles), dim3(256), lds, s, g, G, rank_out, ldr, n_live_out);
    }
    return gd_launch_status("gdmcf_score_rank_f32");
}

}  // extern "C"
