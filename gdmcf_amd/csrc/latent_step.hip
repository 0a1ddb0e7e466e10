// gdmcf_latent_step_f32: one reverse-diffusion step carried in the first hidden layer's space (gfx950 only).
//
//   s[b,n] = sum_k A[b,k] M[n,k];   p_next = c1[b] (s + v[n]) + c2[b] p_cur[b,n];   h_next = act(p_next + e[n])
//
// The shape class is B from 1 to a few thousand, N about 1000, K 1000..3000: a 400 x 1000 output is 0.8 GFLOP over 6 MB of
// operands that sit in L2 / Infinity Cache, and the tiles of the big products (80 x 176 and up) would put 30 workgroups on 256
// CUs.  Here a workgroup of four waves owns a 16 (batch rows) x 64 (columns) output tile and the four waves share its K:
//   * v_mfma_f32_16x16x4_f32 with M as the A operand and the activations as the B operand (D = M A^T), so that a lane's four
//     accumulator registers are four CONSECUTIVE columns n of one batch row: the epilogue loads v, e, p_cur and stores p_next,
//     h_next sixteen bytes at a time.  Four accumulator tiles (64 columns) per wave: four independent MFMA chains.
//   * both operands are K-contiguous, so a lane's operand is one 16-byte load: lane l reads k0 + 4 (l >> 4) .. + 3 of row l & 15
//     and feeds element j to the MFMA of step j.  The MFMA's k slot q = l >> 4 therefore holds k0 + j + 4 q -- the same
//     permutation on both operands, hence a plain (reordered) dot product.  Straight from L2 into registers, no LDS staging: an
//     operand row is read by one wave of this workgroup only.
//   * K is cut into chunks of 16; chunk c goes to wave c % 4 (the four waves walk the rows' 256-byte stretches together).  The
//     four partial tiles meet in LDS (16 KB) and wave w finishes columns 16 w .. 16 w + 15: s = ((s_0 + s_1) + s_2) + s_3,
//     then the epilogue on that sum.  A fixed order, no atomics, no workspace: the same bits on every run (the order is
//     documented at the declaration).  400 x 1000 gives 25 x 16 = 400 workgroups = 1600 waves for the chip's 1024 SIMDs.
//   * tails: rows past B / N are clamped for the loads (their results are never stored), the last partial chunk and every chunk of
//     an operand whose rows are not 16-byte aligned go through guarded scalar loads; stores and the epilogue's loads fall back to
//     scalars per pointer.
//
// gdmcf_latent_step_ex_f32 is a second instantiation of the same kernel template (LatentArgsEx) with two optional parts:
//   * a per-row addend r [B, ldr] in front of the time row: h_next = act((p_next + r[b,n]) + e[n]) (DNNCat's W1x u);
//   * an accumulator over the activations, q_next[b,k] = fma(qa[b], q_cur[b,k], qb[b] * A[b,k]) for k < K (the eps target's Q).
//     Chunk c of A's rows b0 .. b0 + 15 already sits in wave c % 4 of EVERY column tile, lane (r, q) holding A[b0 + r, 16 c + 4 q .. + 3]:
//     the rounds of four chunks are dealt to the column tiles in contiguous runs, and the tile that owns a round writes its 64
//     elements per row from the operand registers -- every element exactly once, plain vector stores, no further load of A.
// The instantiation behind gdmcf_latent_step_f32 (LatentArgs) compiles none of this: its instruction stream is the one it had.
// gdmcf_latent_acc_f32 is the accumulator alone (the last step, where no step kernel runs): the same expression, the same bits.
#include <type_traits>

#include "common.h"
#include "gemm_epilogue.h"

namespace {

constexpr int LS_WAVES = 4;
constexpr int LS_THREADS = 64 * LS_WAVES;
constexpr int LS_TB = 16;  // batch rows per workgroup
constexpr int LS_TN = 64;  // columns per workgroup (four 16-column MFMA tiles)
constexpr int LS_KC = 16;  // k per chunk: one 16-byte load per lane and operand row

struct LatentArgs {
    const float* A;
    int64_t lda;
    const float* M;
    int64_t ldm;
    const float* v;
    const float* p_cur;
    int64_t ldpc;
    const float* c1;
    const float* c2;
    const float* e;
    int act;
    int B, N, K;
    float* p_next;
    int64_t ldpn;
    float* h_next;
    int64_t ldh;
    int ab_vec;  // rows of A and of M are 16-byte aligned: whole chunks by one 16-byte load per lane
    int v_vec, e_vec, pc_vec, pn_vec, h_vec;  // 16-byte accesses allowed on these pointers' rows
};

// four consecutive elements at p[i .. i + 3], i a multiple of four, of a row of n elements
__device__ __forceinline__ f32x4 ls_load4(const float* p, int i, int n, bool vec) {
    if (vec && i + 3 < n) return *reinterpret_cast<const f32x4*>(p + i);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (i + c < n) r[c] = p[i + c];
    return r;
}

__device__ __forceinline__ void ls_store4(float* p, int i, int n, bool vec, f32x4 x) {
    if (vec && i + 3 < n) {
        *reinterpret_cast<f32x4*>(p + i) = x;
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (i + c < n) p[i + c] = x[c];
}

struct LatentArgsEx : LatentArgs {
    const float* r;  // [B, ldr] or NULL
    int64_t ldr;
    const float* q_cur;  // [B, ldqc]
    int64_t ldqc;
    const float* qa;
    const float* qb;
    float* q_next;  // [B, ldqn] or NULL: no accumulator
    int64_t ldqn;
    int r_vec, qc_vec, qn_vec;
};

// q_next[b, k .. k + 3] = fma(qa, q_cur[b, k .. k + 3], qb * a), k a multiple of four; elements at or past K are neither read nor written
__device__ __forceinline__ void ls_acc(const float* q_cur, bool qc_vec, float* q_next, bool qn_vec, int k, int K, float qa, float qb,
                                       const f32x4 a) {
#pragma clang fp contract(off)
    f32x4 qc = {0.f, 0.f, 0.f, 0.f};
    if (qa != 0.f) qc = ls_load4(q_cur, k, K, qc_vec);
    f32x4 qn;
#pragma unroll
    for (int j = 0; j < 4; ++j) qn[j] = __builtin_fmaf(qa, qc[j], qb * a[j]);
    ls_store4(q_next, k, K, qn_vec, qn);
}

struct LsFrag {
    f32x4 a;
    f32x4 m[4];
};

__device__ __forceinline__ void ls_load(LsFrag& f, const float* arow, const float* const (&mrow)[4], int k) {
    f.a = *reinterpret_cast<const f32x4*>(arow + k);
#pragma unroll
    for (int t = 0; t < 4; ++t) f.m[t] = *reinterpret_cast<const f32x4*>(mrow[t] + k);
}

__device__ __forceinline__ void ls_chunk(f32x4 (&acc)[4], const f32x4 a, const f32x4 (&m)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(m[t][j], a[j], acc[t], 0, 0, 0);
}

template <class Args>
__global__ __launch_bounds__(LS_THREADS) void latent_step_kernel(const Args g) {
#pragma clang fp contract(off)
    constexpr bool EX = std::is_same<Args, LatentArgsEx>::value;
    __shared__ f32x4 s_part[LS_WAVES][4][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * LS_TN, b0 = blockIdx.y * LS_TB;
    // operand rows of this lane; a row past the end is the last one again (loaded, multiplied, never stored)
    const int brow = b0 + r < g.B ? b0 + r : g.B - 1;
    const float* arow = g.A + (int64_t)brow * g.lda;
    const float* mrow[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int nrow = n0 + 16 * t + r < g.N ? n0 + 16 * t + r : g.N - 1;
        mrow[t] = g.M + (int64_t)nrow * g.ldm;
    }
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the accumulator (EX): this column tile writes the rounds of four chunks own_lo <= c / 4 < own_hi
    int own_lo = 0, own_hi = 0;
    float qa = 0.f, qb = 0.f;
    const float* qcrow = nullptr;
    float* qnrow = nullptr;
    bool qc_vec = false, qn_vec = false;
    if constexpr (EX) {
        if (g.q_next && b0 + r < g.B) {
            const int rounds = ((g.K + LS_KC - 1) / LS_KC + LS_WAVES - 1) / LS_WAVES;
            const int per = (rounds + (int)gridDim.x - 1) / (int)gridDim.x;
            own_lo = (int)blockIdx.x * per;
            own_hi = own_lo + per;  // (a round past the last one does not occur below)
            qa = g.qa[brow];
            qb = g.qb[brow];
            qcrow = g.q_cur + (int64_t)brow * g.ldqc;
            qnrow = g.q_next + (int64_t)brow * g.ldqn;
            qc_vec = g.qc_vec != 0;
            qn_vec = g.qn_vec != 0;
        }
    }

    int c = wave;
    const int nfull = g.ab_vec ? g.K / LS_KC : 0;  // chunks that end inside K and may be read 16 bytes at a time
    if (c < nfull) {
        // two chunks per round, the next round's ten loads issued before this round's 32 MFMAs (at 1600 waves on 1024 SIMDs there
        // is little else to hide L2 latency behind).  A chunk index past the end is clamped for the load -- every load is issued,
        // none sits behind a branch -- and skipped for the MFMAs.
        const int last = nfull - 1;
        LsFrag f0, f1;
        ls_load(f0, arow, mrow, (c < last ? c : last) * LS_KC + 4 * q);
        ls_load(f1, arow, mrow, (c + LS_WAVES < last ? c + LS_WAVES : last) * LS_KC + 4 * q);
        for (;;) {
            LsFrag g0, g1;
            ls_load(g0, arow, mrow, (c + 2 * LS_WAVES < last ? c + 2 * LS_WAVES : last) * LS_KC + 4 * q);
            ls_load(g1, arow, mrow, (c + 3 * LS_WAVES < last ? c + 3 * LS_WAVES : last) * LS_KC + 4 * q);
            ls_chunk(acc, f0.a, f0.m);
            if (c + LS_WAVES < nfull) ls_chunk(acc, f1.a, f1.m);
            if constexpr (EX) {
                const int rd = c / LS_WAVES;
                if (rd >= own_lo && rd < own_hi) ls_acc(qcrow, qc_vec, qnrow, qn_vec, c * LS_KC + 4 * q, g.K, qa, qb, f0.a);
                if (c + LS_WAVES < nfull && rd + 1 >= own_lo && rd + 1 < own_hi)
                    ls_acc(qcrow, qc_vec, qnrow, qn_vec, (c + LS_WAVES) * LS_KC + 4 * q, g.K, qa, qb, f1.a);
            }
            c += 2 * LS_WAVES;
            if (c >= nfull) break;
            f0 = g0;
            f1 = g1;
        }
        c = wave + (nfull - wave + LS_WAVES - 1) / LS_WAVES * LS_WAVES;  // this wave's first chunk behind the whole ones
    }
    const int nchunks = (g.K + LS_KC - 1) / LS_KC;
    for (; c < nchunks; c += LS_WAVES) {  // the partial last chunk; every chunk of unaligned operands
        const int k = c * LS_KC + 4 * q;
        const f32x4 a = ls_load4(arow, k, g.K, false);
        f32x4 m[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) m[t] = ls_load4(mrow[t], k, g.K, false);
        ls_chunk(acc, a, m);
        if constexpr (EX) {
            if (c / LS_WAVES >= own_lo && c / LS_WAVES < own_hi) ls_acc(qcrow, qc_vec, qnrow, qn_vec, k, g.K, qa, qb, a);
        }
    }

#pragma unroll
    for (int t = 0; t < 4; ++t) s_part[wave][t][lane] = acc[t];
    __syncthreads();
    f32x4 s = s_part[0][wave][lane];
#pragma unroll
    for (int w = 1; w < LS_WAVES; ++w) s += s_part[w][wave][lane];

    // D = M A^T: accumulator register j of lane l is column n0 + 16 t + 4 (l >> 4) + j of batch row b0 + (l & 15)
    const int b = b0 + r, nb = n0 + 16 * wave + 4 * q;
    if (b >= g.B || nb >= g.N) return;
    const float c1 = g.c1[b], c2 = g.c2[b];
    if (g.v) s += ls_load4(g.v, nb, g.N, g.v_vec != 0);
    f32x4 pc = {0.f, 0.f, 0.f, 0.f};
    if (c2 != 0.f) pc = ls_load4(g.p_cur + (int64_t)b * g.ldpc, nb, g.N, g.pc_vec != 0);
    f32x4 p;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = __builtin_fmaf(c2, pc[j], c1 * s[j]);
    ls_store4(g.p_next + (int64_t)b * g.ldpn, nb, g.N, g.pn_vec != 0, p);
    if (!g.h_next) return;
    if constexpr (EX) {
        if (g.r) p += ls_load4(g.r + (int64_t)b * g.ldr, nb, g.N, g.r_vec != 0);
    }
    if (g.e) p += ls_load4(g.e, nb, g.N, g.e_vec != 0);
    if (g.act == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = gd_tanh(p[j]);
    }
    ls_store4(g.h_next + (int64_t)b * g.ldh, nb, g.N, g.h_vec != 0, p);
}

// the accumulator alone: one thread per four consecutive k of a row
__global__ __launch_bounds__(256) void latent_acc_kernel(const float* q_cur, int64_t ldqc, const float* qa, const float* A, int64_t lda,
                                                         const float* qb, int B, int K, float* q_next, int64_t ldqn, int a_vec,
                                                         int qc_vec, int qn_vec) {
    const int k4 = (K + 3) / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * k4) return;
    const int b = (int)(i / k4), k = 4 * (int)(i % k4);
    const f32x4 a = ls_load4(A + (int64_t)b * lda, k, K, a_vec != 0);
    ls_acc(q_cur + (int64_t)b * ldqc, qc_vec != 0, q_next + (int64_t)b * ldqn, qn_vec != 0, k, K, qa[b], qb[b], a);
}

int ls_check(const float* A, int64_t lda, const float* M, int64_t ldm, const float* p_cur, int64_t ldpc,
             const float* c1, const float* c2, int act, int B, int N, int K, float* p_next, int64_t ldpn, float* h_next, int64_t ldh) {
    GD_CHECK_SHAPE(B > 0 && N > 0 && K > 0, "latent_step: empty product");
    GD_CHECK_SHAPE(B <= 65535 * LS_TB, "latent_step: too many rows in one launch");
    GD_CHECK_ARG(A && M && p_cur && c1 && c2 && p_next, "latent_step: A / M / p_cur / c1 / c2 / p_next missing");
    GD_CHECK_ARG(act == 0 || act == 1, "latent_step: act must be 0 (none) or 1 (tanh)");
    GD_CHECK_SHAPE(lda >= K && ldm >= K, "latent_step: lda / ldm below K");
    GD_CHECK_SHAPE(ldpc >= N && ldpn >= N && (!h_next || ldh >= N), "latent_step: leading dimension of p_cur / p_next / h_next below N");
    return 0;
}

void ls_fill(LatentArgs& g, const float* A, int64_t lda, const float* M, int64_t ldm, const float* v, const float* p_cur, int64_t ldpc,
             const float* c1, const float* c2, const float* e, int act, int B, int N, int K, float* p_next, int64_t ldpn,
             float* h_next, int64_t ldh) {
    g.A = A; g.lda = lda; g.M = M; g.ldm = ldm; g.v = v; g.p_cur = p_cur; g.ldpc = ldpc; g.c1 = c1; g.c2 = c2; g.e = e;
    g.act = act; g.B = B; g.N = N; g.K = K; g.p_next = p_next; g.ldpn = ldpn; g.h_next = h_next; g.ldh = ldh;
    g.ab_vec = gd_aligned16(A) && gd_aligned16(M) && (lda % 4) == 0 && (ldm % 4) == 0;
    g.v_vec = v && gd_aligned16(v);
    g.e_vec = e && gd_aligned16(e);
    g.pc_vec = gd_aligned16(p_cur) && (ldpc % 4) == 0;
    g.pn_vec = gd_aligned16(p_next) && (ldpn % 4) == 0;
    g.h_vec = h_next && gd_aligned16(h_next) && (ldh % 4) == 0;
}

}  // namespace

extern "C" {

size_t gdmcf_latent_step_ws_bytes(int B, int N, int K) {
    (void)B; (void)N; (void)K;
    return 0;  // the partial sums of a tile meet in LDS
}

int gdmcf_latent_step_f32(const float* A, int64_t lda, const float* M, int64_t ldm, const float* v, const float* p_cur,
                          int64_t ldpc, const float* c1, const float* c2, const float* e, int act, int B, int N, int K,
                          float* p_next, int64_t ldpn, float* h_next, int64_t ldh, void* ws, size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;
    if (int rc = ls_check(A, lda, M, ldm, p_cur, ldpc, c1, c2, act, B, N, K, p_next, ldpn, h_next, ldh)) return rc;
    LatentArgs g;
    ls_fill(g, A, lda, M, ldm, v, p_cur, ldpc, c1, c2, e, act, B, N, K, p_next, ldpn, h_next, ldh);
    hipLaunchKernelGGL(latent_step_kernel<LatentArgs>, dim3(gd_cdiv(N, LS_TN), gd_cdiv(B, LS_TB)), dim3(LS_THREADS), 0, (hipStream_t)stream, g);
    return gd_launch_status("latent_step");
}

int gdmcf_latent_step_ex_f32(const float* A, int64_t lda, const float* M, int64_t ldm, const float* v, const float* p_cur,
                             int64_t ldpc, const float* c1, const float* c2, const float* r, int64_t ldr, const float* e, int act,
                             int B, int N, int K, float* p_next, int64_t ldpn, float* h_next, int64_t ldh, const float* q_cur,
                             int64_t ldqc, const float* qa, const float* qb, float* q_next, int64_t ldqn, void* ws, size_t ws_bytes,
                             void* stream) {
    (void)ws; (void)ws_bytes;
    if (int rc = ls_check(A, lda, M, ldm, p_cur, ldpc, c1, c2, act, B, N, K, p_next, ldpn, h_next, ldh)) return rc;
    GD_CHECK_SHAPE(!r || ldr >= N, "latent_step_ex: ldr below N");
    GD_CHECK_ARG(!q_next || (q_cur && qa && qb), "latent_step_ex: q_next without q_cur / qa / qb");
    GD_CHECK_SHAPE(!q_next || (ldqc >= K && ldqn >= K), "latent_step_ex: ldq below K");
    GD_CHECK_ARG(!q_next || q_next != A, "latent_step_ex: q_next must not be A (other column tiles still read it)");
    LatentArgsEx g;
    ls_fill(g, A, lda, M, ldm, v, p_cur, ldpc, c1, c2, e, act, B, N, K, p_next, ldpn, h_next, ldh);
    g.r = r; g.ldr = ldr; g.q_cur = q_cur; g.ldqc = ldqc; g.qa = qa; g.qb = qb; g.q_next = q_next; g.ldqn = ldqn;
    g.r_vec = r && gd_aligned16(r) && (ldr % 4) == 0;
    g.qc_vec = q_next && gd_aligned16(q_cur) && (ldqc % 4) == 0;
    g.qn_vec = q_next && gd_aligned16(q_next) && (ldqn % 4) == 0;
    hipLaunchKernelGGL(latent_step_kernel<LatentArgsEx>, dim3(gd_cdiv(N, LS_TN), gd_cdiv(B, LS_TB)), dim3(LS_THREADS), 0, (hipStream_t)stream, g);
    return gd_launch_status("latent_step_ex");
}

int gdmcf_latent_acc_f32(const float* q_cur, int64_t ldqc, const float* qa, const float* A, int64_t lda, const float* qb, int B, int K,
                         float* q_next, int64_t ldqn, void* stream) {
    GD_CHECK_SHAPE(B > 0 && K > 0, "latent_acc: empty update");
    GD_CHECK_ARG(q_cur && qa && A && qb && q_next, "latent_acc: q_cur / qa / A / qb / q_next missing");
    GD_CHECK_SHAPE(lda >= K && ldqc >= K && ldqn >= K, "latent_acc: lda / ldq below K");
    GD_CHECK_ARG(q_next != A, "latent_acc: q_next must not be A");
    const int64_t n = (int64_t)B * ((K + 3) / 4);
    GD_CHECK_SHAPE((n + 255) / 256 <= 0x7fffffff, "latent_acc: too many elements in one launch");
    hipLaunchKernelGGL(latent_acc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q_cur, ldqc, qa, A, lda, qb,
                       B, K, q_next, ldqn, gd_aligned16(A) && (lda % 4) == 0, gd_aligned16(q_cur) && (ldqc % 4) == 0,
                       gd_aligned16(q_next) && (ldqn % 4) == 0);
    return gd_launch_status("latent_acc");
}

}  // extern "C"
