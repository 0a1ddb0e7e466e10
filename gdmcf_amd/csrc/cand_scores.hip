// Candidate scoring (gdmcf_amd.score_candidates / recommend(candidates=); gfx950 only).
//
// gdmcf_cand_scores_f32:  out[b, c] = (dot(A[b, :K], W[cand[b, c], :K]) + bias[cand[b, c]]) * scale[b]
// gdmcf_cand_pick_f32:    out[b, c] = dense[b, cand[b, c]] * scale[b]
// both with -inf for a candidate outside [0, I) or listed in row rows[b] of either mask CSR.
//
// The gathered product is bound by the row reads (K * 4 bytes per candidate out of a table that sits in the Infinity Cache), so
// it runs on the vector ALUs:
//   * one wave per (user, run of S <= 64 consecutive list positions); four waves to a workgroup, none of them talks to another
//     (no LDS, no barrier).  S comes from B * C on the host so that small calls still spread over the chip (cs_run_length).
//   * the wave stages its run one candidate per lane, range-checks it, and tests it against the user's mask rows: the mask's
//     indices are read 64 at a time, one per lane, and every candidate of the run is broadcast against them (v_readlane, one
//     ballot each).  Dead candidates get their -inf here and take no further part: no row of W and no bias is read for them.
//   * the user's row of A stays in registers, lane l holding k = 256 j + 4 l .. + 3 for j < NJ = ceil(K / 256) (at most 16 f32x4).
//   * the live candidates are taken four at a time (their lanes from the ballot, their ids by v_readlane: the row pointers are
//     wave-uniform).  A row is read as NJ fully coalesced 1-KB instructions, four rows are in flight per wave.  A last group of
//     fewer than four repeats its first row in the free slots (computed, not stored).
//   * summation order (the same for every candidate, wherever it stands in its list): lane l adds its products in ascending k
//     into one accumulator, acc = fma(a[k], w[k], acc) from +0; the 64 accumulators meet in a butterfly over the lane masks
//     32, 16, 8, 4, 2, 1 in that order, x = x(l) + x(l ^ m) -- an addition whose operands trade places between the two lanes
//     and whose result therefore has the same bits in both.  The first two levels fold the group's four candidates together
//     (each lane hands over the two, then the one, it does not keep), so four candidates cost 7 cross-lane moves, not 24, and
//     candidate g of the group ends in lanes 16 g .. 16 g + 15.  Then (sum + bias) * scale, two roundings.
//   * tails: the last 256-wide piece of K, and every piece when a row of A or W is not 16-byte aligned or K is no multiple of
//     four, go through guarded loads without a branch (cs_load4: the index clamped, the value replaced by zero; fma(0, 0, acc) is
//     acc); elements at or past K are never read.
// No atomics, no workspace, no host synchronisation.
#include "common.h"

namespace {

constexpr int CS_WAVES = 4;
constexpr int CS_THREADS = 64 * CS_WAVES;
constexpr int CS_GROUP = 4;        // candidate rows in flight per wave
constexpr int CS_MAX_K = 4096;     // 16 f32x4 of A per lane
constexpr int64_t CS_WAVES_WANTED = 4096;  // 256 CUs x 16 waves: run lengths grow only once the call fills the chip

struct CandMask {
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* indptr2;
    const int32_t* indices2;
    const int64_t* rows;  // [B] row of both CSRs per output row (nullptr: the output row's own number)
};

struct CandList {
    const int64_t* cand;
    int64_t ldcand;  // 0: one list for every row
    int C;
    int S;           // list positions per wave (<= 64)
    int nseg;        // ceil(C / S)
    int64_t n_work;  // B * nseg
    int I;
};

// bit s set: candidate `readlane(cid, s)` (s < n) occurs in CSR row r.  The row's indices 64 at a time, one per lane.
__device__ __forceinline__ uint64_t cs_row_hits(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t r,
                                                int cid, int n, int lane) {
    uint64_t hits = 0;
    const int64_t beg = indptr[r], end = indptr[r + 1];
    for (int64_t base = beg; base < end; base += 64) {
        const int m = base + lane < end ? indices[base + lane] : -1;
        for (int s = 0; s < n; ++s) {
            const int c = __builtin_amdgcn_readlane(cid, s);
            if (__ballot(m == c) != 0ull) hits |= 1ull << s;
        }
    }
    return hits;
}

// The wave's run of the list: which output row, where the run starts, this lane's candidate (-1: none, out of range or masked --
// then -inf has been stored for it, if the lane has a list position at all).  Returns false for a wave without work.
__device__ __forceinline__ bool cs_stage(const CandList& L, const CandMask& M, float* __restrict__ out, int64_t ldo, int lane,
                                         int64_t& b, float*& orow, int& cid) {
    const int64_t wid = (int64_t)blockIdx.x * CS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wid >= L.n_work) return false;
    b = wid / L.nseg;
    const int c0 = (int)(wid - b * L.nseg) * L.S;
    const int n = L.C - c0 < L.S ? L.C - c0 : L.S;
    cid = -1;
    if (lane < n) {
        const int64_t c = L.cand[b * L.ldcand + c0 + lane];
        if (c >= 0 && c < (int64_t)L.I) cid = (int)c;
    }
    if (M.indptr) {
        const int64_t mr = M.rows ? M.rows[b] : b;
        uint64_t hits = cs_row_hits(M.indptr, M.indices, mr, cid, n, lane);
        if (M.indptr2) hits |= cs_row_hits(M.indptr2, M.indices2, mr, cid, n, lane);
        if ((hits >> lane) & 1ull) cid = -1;  // (a lane without a candidate matches the filler -1: it is dead already)
    }
    orow = out + b * ldo + c0;
    if (lane < n && cid < 0) orow[lane] = -__builtin_inff();
    return true;
}

// p[k .. k + 3] of a row of K elements, zeros at and past K, without a branch (the j loop stays one basic block, so its stages
// stay where they are written).  WHOLE: k + 3 < K in every lane.  VEC: the row is 16-byte aligned and K a multiple of four, so a
// lane's four elements lie before K or past it together -- one 16-byte load, from the row's start in the lanes past K.  Otherwise
// four scalar loads, those at and past K from element K - 1 instead.  Nothing at or past K is read either way.
template <bool VEC, bool WHOLE>
__device__ __forceinline__ f32x4 cs_load4(const float* __restrict__ p, int k, int K) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if (VEC) {
        const bool ok = WHOLE || k < K;
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + (ok ? k : 0));
        return ok ? v : zero;
    }
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool ok = WHOLE || k + c < K;
        const float v = p[ok ? k + c : K - 1];
        r[c] = ok ? v : 0.f;
    }
    return r;
}

struct CandScoreArgs {
    const float* A;
    int64_t lda;
    const float* W;
    int64_t ldw;
    int K;
    const float* bias;
    const float* scale;
    float* out;
    int64_t ldo;
    CandList L;
    CandMask M;
};

// VEC: the rows of A and of W are 16-byte aligned and K is a multiple of four.  The j loop is cut into stages of P pieces -- P x 4
// rows x 16 bytes per lane in flight, then their FMAs -- so that the loads of a stage are issued together and the budget of four
// waves per SIMD (16 per CU) holds up to K = 4096: 64 registers of A beside 32 of loads.  (Left alone hipcc hoists all 4 NJ loads:
// one wave per SIMD from K = 2816.)
template <int NJ, bool VEC>
__global__ __launch_bounds__(CS_THREADS) void cand_scores_kernel(const CandScoreArgs g) {
#pragma clang fp contract(off)
    constexpr int P = NJ <= 8 ? (NJ < 4 ? NJ : 4) : 2;
    const int lane = threadIdx.x & 63;
    int64_t b;
    float* orow;
    int cid;
    if (!cs_stage(g.L, g.M, g.out, g.ldo, lane, b, orow, cid)) return;
    uint64_t todo = __ballot(cid >= 0);
    if (todo == 0ull) return;

    const int K = g.K;
    // pieces j < NJ - 1 are whole (K > 256 (NJ - 1)); in the last one a lane's four elements may cross K
    const float* arow = g.A + b * g.lda;
    f32x4 a[NJ];
#pragma unroll
    for (int j = 0; j < NJ - 1; ++j) a[j] = cs_load4<VEC, true>(arow, 256 * j + 4 * lane, K);
    a[NJ - 1] = cs_load4<VEC, false>(arow, 256 * (NJ - 1) + 4 * lane, K);
    const int q = lane >> 4;

    while (todo != 0ull) {
        int pos[CS_GROUP], id[CS_GROUP];
        const float* w[CS_GROUP];
        int cnt = 0;
#pragma unroll
        for (int t = 0; t < CS_GROUP; ++t) {
            if (todo != 0ull) {
                pos[t] = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                ++cnt;
            } else {
                pos[t] = pos[0];
            }
            id[t] = __builtin_amdgcn_readlane(cid, pos[t]);
            w[t] = g.W + (int64_t)id[t] * g.ldw;
        }
        float acc[CS_GROUP] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j0 = 0; j0 < NJ; j0 += P) {
            f32x4 x[P][CS_GROUP];
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int t = 0; t < CS_GROUP; ++t) {
                    const int j = j0 + p;
                    if (j < NJ - 1) x[p][t] = cs_load4<VEC, true>(w[t], 256 * j + 4 * lane, K);
                    else if (j == NJ - 1) x[p][t] = cs_load4<VEC, false>(w[t], 256 * j + 4 * lane, K);
                }
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int t = 0; t < CS_GROUP; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (j0 + p < NJ) acc[t] = __builtin_fmaf(a[j0 + p][c], x[p][t][c], acc[t]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // masks 32 and 16 fold the four candidates: lanes < 32 keep 0 and 1, then lanes with bit 4 clear keep the lower of their two
        const bool hi = (lane & 32) != 0;
        const float x0 = (hi ? acc[2] : acc[0]) + __shfl_xor(hi ? acc[0] : acc[2], 32);
        const float x1 = (hi ? acc[3] : acc[1]) + __shfl_xor(hi ? acc[1] : acc[3], 32);
        const bool h2 = (lane & 16) != 0;
        float y = (h2 ? x1 : x0) + __shfl_xor(h2 ? x0 : x1, 16);
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) y = y + __shfl_xor(y, m);
        if ((lane & 15) == 0 && q < cnt) {
            const int my_id = q == 0 ? id[0] : q == 1 ? id[1] : q == 2 ? id[2] : id[3];
            const int my_pos = q == 0 ? pos[0] : q == 1 ? pos[1] : q == 2 ? pos[2] : pos[3];
            float r = y;
            if (g.bias) r = r + g.bias[my_id];
            if (g.scale) r = r * g.scale[b];
            orow[my_pos] = r;
        }
    }
}

struct CandPickArgs {
    const float* dense;
    int64_t ldd;
    const float* scale;
    float* out;
    int64_t ldo;
    CandList L;
    CandMask M;
};

__global__ __launch_bounds__(CS_THREADS) void cand_pick_kernel(const CandPickArgs g) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    int64_t b;
    float* orow;
    int cid;
    if (!cs_stage(g.L, g.M, g.out, g.ldo, lane, b, orow, cid)) return;
    if (cid < 0) return;
    float r = g.dense[b * g.ldd + cid];
    if (g.scale) r = r * g.scale[b];
    orow[lane] = r;
}

// List positions per wave: a multiple of the group of four, as short as it takes to put CS_WAVES_WANTED waves on the chip, at most
// the 64 a wave stages at once (16 users x 100 candidates: 4, 400 waves; 400 x 100: 12, 3 600 waves).
int cs_run_length(int64_t B, int64_t C) {
    int64_t s = (B * C + CS_WAVES_WANTED - 1) / CS_WAVES_WANTED;
    s = (s + CS_GROUP - 1) / CS_GROUP * CS_GROUP;
    return (int)(s < CS_GROUP ? CS_GROUP : s > 64 ? 64 : s);
}

int cs_common(const char* what, const int64_t* cand, int64_t ldcand, int B, int C, int I, int S, const int64_t* indptr,
              const int32_t* indices, const int64_t* indptr2, const int32_t* indices2, const int64_t* rows, const float* out,
              int64_t ldo, CandList& L, CandMask& M, unsigned& grid) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: bad shape (B > 0, C > 0, I > 0, ldo >= C, ldcand == 0 or >= C)", what);
    GD_CHECK_SHAPE(B > 0 && C > 0 && I > 0 && ldo >= C && (ldcand == 0 || ldcand >= C), msg);
    snprintf(msg, sizeof msg, "%s: mask indptr/indices mismatch, or a second CSR without the first", what);
    GD_CHECK_ARG((indptr == nullptr) == (indices == nullptr) && (indptr2 == nullptr) == (indices2 == nullptr) &&
                     (indptr2 == nullptr || indptr != nullptr), msg);
    snprintf(msg, sizeof msg, "%s: null cand / out", what);
    GD_CHECK_ARG(cand && out, msg);
    L.cand = cand;
    L.ldcand = ldcand;
    L.C = C;
    L.S = S;
    L.nseg = (C + S - 1) / S;
    L.n_work = (int64_t)B * L.nseg;
    L.I = I;
    M = CandMask{indptr, indices, indptr2, indices2, rows};
    const int64_t blocks = (L.n_work + CS_WAVES - 1) / CS_WAVES;
    snprintf(msg, sizeof msg, "%s: B * C too large for one launch", what);
    GD_CHECK_ARG(blocks <= 0x7fffffffll, msg);
    grid = (unsigned)blocks;
    return GDMCF_OK;
}

}  // namespace

extern "C" {

int gdmcf_cand_scores_f32(const float* A, int64_t lda, const float* W, int64_t ldw, int I, int K, const float* bias,
                          const float* scale, const int64_t* cand, int64_t ldcand, int B, int C, const int64_t* indptr,
                          const int32_t* indices, const int64_t* indptr2, const int32_t* indices2, const int64_t* rows, float* out,
                          int64_t ldo, void* stream) {
    GD_CHECK_SHAPE(K >= 1 && K <= CS_MAX_K, "gdmcf_cand_scores_f32: K out of range (1 <= K <= 4096)");
    GD_CHECK_SHAPE(lda >= K && ldw >= K, "gdmcf_cand_scores_f32: bad shape (lda >= K, ldw >= K)");
    CandScoreArgs g;
    unsigned grid;
    const int rc = cs_common("gdmcf_cand_scores_f32", cand, ldcand, B, C, I, cs_run_length(B > 0 ? B : 1, C > 0 ? C : 1), indptr,
                             indices, indptr2, indices2, rows, out, ldo, g.L, g.M, grid);
    if (rc != GDMCF_OK) return rc;
    GD_CHECK_ARG(A && W, "gdmcf_cand_scores_f32: null A / W");
    g.A = A;
    g.lda = lda;
    g.W = W;
    g.ldw = ldw;
    g.K = K;
    g.bias = bias;
    g.scale = scale;
    g.out = out;
    g.ldo = ldo;
    const bool vec = gd_aligned16(A) && lda % 4 == 0 && gd_aligned16(W) && ldw % 4 == 0 && K % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    switch ((K + 255) / 256) {
#define CS_CASE(NJ)                                                                                      \
    case NJ:                                                                                             \
        if (vec) hipLaunchKernelGGL((cand_scores_kernel<NJ, true>), dim3(grid), dim3(CS_THREADS), 0, s, g); \
        else hipLaunchKernelGGL((cand_scores_kernel<NJ, false>), dim3(grid), dim3(CS_THREADS), 0, s, g);    \
        break;
        CS_CASE(1) CS_CASE(2) CS_CASE(3) CS_CASE(4) CS_CASE(5) CS_CASE(6) CS_CASE(7) CS_CASE(8)
        CS_CASE(9) CS_CASE(10) CS_CASE(11) CS_CASE(12) CS_CASE(13) CS_CASE(14) CS_CASE(15) CS_CASE(16)
#undef CS_CASE
    }
    return gd_launch_status("gdmcf_cand_scores_f32");
}

int gdmcf_cand_pick_f32(const float* dense, int64_t ldd, int B, int I, const float* scale, const int64_t* cand, int64_t ldcand,
                        int C, const int64_t* indptr, const int32_t* indices, const int64_t* indptr2, const int32_t* indices2,
                        const int64_t* rows, float* out, int64_t ldo, void* stream) {
    GD_CHECK_SHAPE(I > 0 && ldd >= I, "gdmcf_cand_pick_f32: bad shape (I > 0, ldd >= I)");
    CandPickArgs g;
    unsigned grid;
    const int rc = cs_common("gdmcf_cand_pick_f32", cand, ldcand, B, C, I, 64, indptr, indices, indptr2, indices2, rows, out, ldo,
                             g.L, g.M, grid);
    if (rc != GDMCF_OK) return rc;
    GD_CHECK_ARG(dense != nullptr, "gdmcf_cand_pick_f32: null dense");
    g.dense = dense;
    g.ldd = ldd;
    g.scale = scale;
    g.out = out;
    g.ldo = ldo;
    hipLaunchKernelGGL(cand_pick_kernel, dim3(grid), dim3(CS_THREADS), 0, (hipStream_t)stream, g);
    return gd_launch_status("gdmcf_cand_pick_f32");
}

}  // extern "C"
