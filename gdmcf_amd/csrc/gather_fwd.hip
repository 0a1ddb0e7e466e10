// gdmcf_gather_fwd_f32: a first hidden layer whose input row is sparse and binary, as a sum of table rows (gfx950 only).
//
// The reverse loop of an evaluation with sampling_steps == 0 starts from x_0 itself: an exactly {0,1} row with a few dozen ones.
// Without dropout the product [x_0 | emb] . W^T is then nnz(row) rows of W^T plus E embedding rows -- a gather of ~60 rows of 4 KB
// instead of a 400 x 34 405 x 1000 GEMM.  The same kernel serves the one-hot backbones' second branch, whose per-batch part (the
// noiseless one-hot image times W2^T) is gathered once (`base` + rows of the difference table) and re-enters every step as `pre`.
//
// One 256-thread workgroup per (batch row, slab of 1024 output columns), one float4 per lane: a table row is one fully coalesced
// 4 KB read per workgroup.  The row's column indices go through LDS 256 at a time; the loop over them is unrolled by GF_UNROLL so
// that many independent row loads are in flight per lane; the sum stays in registers and is taken in index order (the order
// documented at the declaration), so every launch gives the same bits.  No atomics, no workspace.
#include "common.h"
#include "gemm_epilogue.h"

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_SLAB = 4 * GF_THREADS;  // output columns per workgroup
constexpr int GF_UNROLL = 8;             // table rows in flight per lane

struct GatherArgs {
    const float* pre;
    int64_t ldpre;
    const float* base;
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* rows;
    const float* table;
    int64_t ldt;
    int I;
    const float* a;
    int64_t lda;
    const float* tblE;
    int64_t ldte;
    int E;
    const float* bias;
    int act;
    int N;
    float* out;
    int64_t ldo;
    int pre_vec, out_vec;  // rows of pre / out are 16-byte aligned: one float4 access per lane (else four scalar ones)
};

// four consecutive elements of a vector or matrix row that need not be 16-byte aligned and may end inside the group
__device__ __forceinline__ f32x4 gf_load4(const float* p, int n0, int N, bool vec) {
    if (vec && n0 + 3 < N) return *reinterpret_cast<const f32x4*>(p + n0);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (n0 + c < N) v[c] = p[n0 + c];
    return v;
}

__global__ __launch_bounds__(GF_THREADS) void gather_fwd_kernel(const GatherArgs g) {
#pragma clang fp contract(off)
    __shared__ int s_idx[GF_THREADS];
    const int b = blockIdx.y;
    const int n0 = blockIdx.x * GF_SLAB + threadIdx.x * 4;
    const bool live = n0 < g.N;  // (a table row is padded to a multiple of four columns: a live lane's float4 stays inside it)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (live && g.pre) acc = gf_load4(g.pre + (int64_t)b * g.ldpre, n0, g.N, g.pre_vec != 0);
    if (live && g.base) acc += gf_load4(g.base, n0, g.N, false);
    if (g.indptr) {
        const int64_t r = g.rows[b];
        const int64_t beg = g.indptr[r], end = g.indptr[r + 1];
        for (int64_t k0 = beg; k0 < end; k0 += GF_THREADS) {
            const int cnt = (int)((end - k0) < (int64_t)GF_THREADS ? (end - k0) : (int64_t)GF_THREADS);
            __syncthreads();  // (the previous chunk has been read)
            if ((int)threadIdx.x < cnt) {
                const int ci = g.indices[k0 + threadIdx.x];
                s_idx[threadIdx.x] = (ci >= 0 && ci < g.I) ? ci : -1;  // an index outside the table adds nothing and reads nothing
            }
            __syncthreads();
            if (live) {
                int k = 0;
                for (; k + GF_UNROLL <= cnt; k += GF_UNROLL) {
                    f32x4 v[GF_UNROLL];
#pragma unroll
                    for (int u = 0; u < GF_UNROLL; ++u) {
                        const int j = __builtin_amdgcn_readfirstlane(s_idx[k + u]);
                        v[u] = *reinterpret_cast<const f32x4*>(g.table + (int64_t)(j < 0 ? 0 : j) * g.ldt + n0);
                        if (j < 0) v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int u = 0; u < GF_UNROLL; ++u) acc += v[u];
                }
                for (; k < cnt; ++k) {
                    const int j = __builtin_amdgcn_readfirstlane(s_idx[k]);
                    if (j >= 0) acc += *reinterpret_cast<const f32x4*>(g.table + (int64_t)j * g.ldt + n0);
                }
            }
        }
    }
    if (!live) return;
    if (g.a) {
        const float* ab = g.a + (int64_t)b * g.lda;
        for (int e = 0; e < g.E; ++e) {
            const float ae = ab[e];
            const f32x4 t = *reinterpret_cast<const f32x4*>(g.tblE + (int64_t)e * g.ldte + n0);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_fmaf(ae, t[c], acc[c]);
        }
    }
    if (g.bias) acc += gf_load4(g.bias, n0, g.N, false);
    if (g.act == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = gd_tanh(acc[c]);
    }
    float* o = g.out + (int64_t)b * g.ldo;
    if (g.out_vec && n0 + 3 < g.N) {
        *reinterpret_cast<f32x4*>(o + n0) = acc;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (n0 + c < g.N) o[n0 + c] = acc[c];
    }
}

}  // namespace

extern "C" {

int gdmcf_gather_fwd_f32(const float* pre, int64_t ldpre, const float* base, const int64_t* indptr, const int32_t* indices,
                         const int64_t* rows, const float* table, int64_t ldt, int I, const float* a, int64_t lda,
                         const float* tblE, int64_t ldte, int E, const float* bias, int act, int B, int N, float* out, int64_t ldo,
                         void* stream) {
    GD_CHECK_SHAPE(B > 0 && N > 0 && E >= 0, "gather_fwd: empty batch");
    GD_CHECK_SHAPE(B <= 65535, "gather_fwd: more than 65535 rows in one launch");
    GD_CHECK_ARG(out != nullptr, "gather_fwd: out missing");
    GD_CHECK_ARG(act == 0 || act == 1, "gather_fwd: act must be 0 (none) or 1 (tanh)");
    const bool gather = indptr != nullptr;
    const bool emb = a != nullptr && E > 0;
    GD_CHECK_ARG(pre || gather || emb, "gather_fwd: nothing to sum (none of pre / CSR rows / a given)");
    GD_CHECK_ARG(!gather || (indices && rows && table), "gather_fwd: CSR arrays / row ids / table missing");
    GD_CHECK_ARG((a != nullptr) == (E > 0) && (!emb || tblE), "gather_fwd: a [B, E] and tblE [E, N] go together with E > 0");
    GD_CHECK_SHAPE(ldo >= N && (!pre || ldpre >= N) && (!emb || lda >= E), "gather_fwd: leading dimension below the row width");
    GD_CHECK_SHAPE(!gather || (I > 0 && ldt >= N && (ldt % 4) == 0 && gd_aligned16(table)),
                   "gather_fwd: table must be 16B aligned with ldt % 4 == 0, ldt >= N");
    GD_CHECK_SHAPE(!emb || (ldte >= N && (ldte % 4) == 0 && gd_aligned16(tblE)),
                   "gather_fwd: tblE must be 16B aligned with ldte % 4 == 0, ldte >= N");
    GatherArgs g;
    g.pre = pre; g.ldpre = ldpre; g.base = base;
    g.indptr = indptr; g.indices = indices; g.rows = rows; g.table = table; g.ldt = ldt; g.I = I;
    g.a = emb ? a : nullptr; g.lda = lda; g.tblE = tblE; g.ldte = ldte; g.E = E;
    g.bias = bias; g.act = act; g.N = N; g.out = out; g.ldo = ldo;
    g.pre_vec = pre && gd_aligned16(pre) && (ldpre % 4) == 0;
    g.out_vec = gd_aligned16(out) && (ldo % 4) == 0;
    hipLaunchKernelGGL(gather_fwd_kernel, dim3(gd_cdiv(N, GF_SLAB), B), dim3(GF_THREADS), 0, (hipStream_t)stream, g);
    return gd_launch_status("gather_fwd");
}

}  // extern "C"
