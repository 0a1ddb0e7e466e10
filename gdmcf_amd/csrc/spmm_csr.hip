// LightGCN propagation, first-generation CSR SpMM (reference lightGCN.py:184-189): one wave per virtual row of a host-built
// plan (gdmcf_amd/spmm_schedule.py:spmm_plan).  Bound by HBM / cache bandwidth.
#include "common.h"
#include "spmm.h"

namespace {

// ---------------------------------------------------------------------------------------------
// CSR SpMM  Y = (A X + sum_k addend_k) * scale,  one wave per VIRTUAL row.
// Degree skew is the problem (a hub item has 1e4+ neighbours, the median row ~20): the host splits
// every row into virtual rows of <= chunk nonzeros (plan arrays below), so hub rows spread over many
// waves; a row that was split writes float partials that a second tiny kernel adds in slot order
// (deterministic, no atomics).  LPR lanes cover one embedding row with 16-byte loads, so a wave
// gathers 64/LPR neighbour rows per instruction (d = 64: 4 x 256 B) and keeps 4 such instructions
// in flight.  The LightGCN layer mean is fused through `addends`/`scale` in the last layer.
// ---------------------------------------------------------------------------------------------

template <int LPR>
__global__ __launch_bounds__(256) void spmm_vec_kernel(const int64_t* __restrict__ vbeg, const int64_t* __restrict__ vend,
                                                       const int32_t* __restrict__ vrow,
                                                       const int32_t* __restrict__ vslot, int n_virtual,
                                                       const int32_t* __restrict__ col,
                                                       const float* __restrict__ val, const float* __restrict__ X,
                                                       int64_t ldx, float* __restrict__ Y, int64_t ldy,
                                                       float* __restrict__ partial, int d, const SpmmAdd add) {
    constexpr int NPAR = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n_virtual) return;
    const int sub = lane / LPR, cl = lane % LPR;
    const int64_t beg = vbeg[v], end = vend[v];
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int64_t j = beg + sub;
    for (; j + 3 * NPAR < end; j += 4 * NPAR) {
        const int c0 = col[j], c1 = col[j + NPAR], c2 = col[j + 2 * NPAR], c3 = col[j + 3 * NPAR];
        const float w0 = val[j], w1 = val[j + NPAR], w2 = val[j + 2 * NPAR], w3 = val[j + 3 * NPAR];
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(X + (int64_t)c0 * ldx + cl * 4);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(X + (int64_t)c1 * ldx + cl * 4);
        const f32x4 x2 = *reinterpret_cast<const f32x4*>(X + (int64_t)c2 * ldx + cl * 4);
        const f32x4 x3 = *reinterpret_cast<const f32x4*>(X + (int64_t)c3 * ldx + cl * 4);
        s0 += w0 * x0;
        s1 += w1 * x1;
        s2 += w2 * x2;
        s3 += w3 * x3;
    }
    for (; j < end; j += NPAR) {
        const int c0 = col[j];
        const float w0 = val[j];
        s0 += w0 * *reinterpret_cast<const f32x4*>(X + (int64_t)c0 * ldx + cl * 4);
    }
    f32x4 s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
        s.x += __shfl_xor(s.x, o);
        s.y += __shfl_xor(s.y, o);
        s.z += __shfl_xor(s.z, o);
        s.w += __shfl_xor(s.w, o);
    }
    if (sub == 0) {
        const int slot = vslot[v];
        if (slot >= 0) {
            *reinterpret_cast<f32x4*>(partial + (int64_t)slot * d + cl * 4) = s;
        } else {
            spmm_store_row(s, add, Y, ldy, vrow[v], cl);
        }
    }
}

// Short rows (the bulk of a user-item graph: median degree ~ 20): LPR lanes own one whole row, so a wave
// works on 64/LPR rows at once.  With one row per wave the kernel is bound by the dependent chain
// vptr -> col/val -> gather -> store of 50 k+ tiny waves (measured 39 us for the user half of the Yelp graph);
// here each lane group fetches up to LPR (col, val) pairs with one coalesced load, broadcasts them with
// group-local shuffles and keeps 4 gathers in flight.  Accumulation is in CSR order (deterministic).
template <int LPR>
__global__ __launch_bounds__(256) void spmm_short_kernel(const int64_t* __restrict__ vbeg, const int64_t* __restrict__ vend,
                                                         const int32_t* __restrict__ vrow, int n_short,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, const float* __restrict__ X,
                                                         int64_t ldx, float* __restrict__ Y, int64_t ldy,
                                                         const SpmmAdd add) {
    constexpr int G = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int grp = lane / LPR, gl = lane % LPR;
    const int v = (blockIdx.x * 4 + (threadIdx.x >> 6)) * G + grp;
    if (v >= n_short) return;  // whole lane group leaves together
    const int64_t beg = vbeg[v], end = vend[v];
    const int r = vrow[v];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int64_t base = beg; base < end; base += LPR) {
        const bool have = base + gl < end;
        const int my_c = have ? col[base + gl] : 0;
        const float my_w = have ? val[base + gl] : 0.f;
        const int n = (int)min((int64_t)LPR, end - base);
        int j = 0;
        for (; j + 3 < n; j += 4) {
            const int c0 = __shfl(my_c, j, LPR), c1 = __shfl(my_c, j + 1, LPR), c2 = __shfl(my_c, j + 2, LPR),
                      c3 = __shfl(my_c, j + 3, LPR);
            const float w0 = __shfl(my_w, j, LPR), w1 = __shfl(my_w, j + 1, LPR), w2 = __shfl(my_w, j + 2, LPR),
                        w3 = __shfl(my_w, j + 3, LPR);
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(X + (int64_t)c0 * ldx + gl * 4);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(X + (int64_t)c1 * ldx + gl * 4);
            const f32x4 x2 = *reinterpret_cast<const f32x4*>(X + (int64_t)c2 * ldx + gl * 4);
            const f32x4 x3 = *reinterpret_cast<const f32x4*>(X + (int64_t)c3 * ldx + gl * 4);
            s += w0 * x0;
            s += w1 * x1;
            s += w2 * x2;
            s += w3 * x3;
        }
        for (; j < n; ++j) {
            const int c0 = __shfl(my_c, j, LPR);
            const float w0 = __shfl(my_w, j, LPR);
            s += w0 * *reinterpret_cast<const f32x4*>(X + (int64_t)c0 * ldx + gl * 4);
        }
    }
    spmm_store_row(s, add, Y, ldy, r, gl);
}

// generic fallback (any d): one neighbour at a time, lanes stride over columns
__global__ __launch_bounds__(256) void spmm_generic_kernel(const int64_t* __restrict__ vbeg, const int64_t* __restrict__ vend,
                                                           const int32_t* __restrict__ vrow,
                                                           const int32_t* __restrict__ vslot, int n_virtual,
                                                           const int32_t* __restrict__ col,
                                                           const float* __restrict__ val, const float* __restrict__ X,
                                                           int64_t ldx, float* __restrict__ Y, int64_t ldy,
                                                           float* __restrict__ partial, int d, const SpmmAdd add) {
    const int lane = threadIdx.x & 63;
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n_virtual) return;
    const int64_t beg = vbeg[v], end = vend[v];
    const int slot = vslot[v], r = vrow[v];
    for (int c0 = lane; c0 < d; c0 += 64) {
        float s = 0.f;
        for (int64_t j = beg; j < end; ++j) s += val[j] * X[(int64_t)col[j] * ldx + c0];
        if (slot >= 0) {
            partial[(int64_t)slot * d + c0] = s;
        } else {
            spmm_store_elem(s, add, Y, ldy, r, c0);
        }
    }
}

// rows that were split: Y[r] = (sum of their partial slots + addends) * scale.  One workgroup per split
// row: wave w adds slots w, w+4, ... (independent loads, 4 in flight), the four partial sums are added in
// wave order -> fixed summation order, no atomics.
__global__ __launch_bounds__(256) void spmm_combine_kernel(const int32_t* __restrict__ lrow,
                                                           const int32_t* __restrict__ lptr, int n_long,
                                                           const float* __restrict__ partial, int d,
                                                           float* __restrict__ Y, int64_t ldy, const SpmmAdd add) {
    extern __shared__ float comb[];  // [4][d]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l = blockIdx.x;
    const int r = lrow[l];
    const int beg = lptr[l], end = lptr[l + 1];
    for (int c0 = lane; c0 < d; c0 += 64) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int k = beg + wave;
        for (; k + 12 < end; k += 16) {
            s0 += partial[(int64_t)k * d + c0];
            s1 += partial[(int64_t)(k + 4) * d + c0];
            s2 += partial[(int64_t)(k + 8) * d + c0];
            s3 += partial[(int64_t)(k + 12) * d + c0];
        }
        for (; k < end; k += 4) s0 += partial[(int64_t)k * d + c0];
        comb[wave * d + c0] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (wave == 0) {
        for (int c0 = lane; c0 < d; c0 += 64) {
            spmm_store_elem(((comb[c0] + comb[d + c0]) + comb[2 * d + c0]) + comb[3 * d + c0], add, Y, ldy, r, c0);
        }
    }
}

}  // namespace

extern "C" {

int gdmcf_spmm_csr_f32(const int64_t* vbeg, const int64_t* vend, const int32_t* vrow, const int32_t* vslot, int n_virtual, int n_short,
                       const int32_t* lrow, const int32_t* lptr, int n_long, const int32_t* col, const float* val,
                       int n_rows, const float* X, int64_t ldx, int d, float* Y, int64_t ldy, float* partial_ws,
                       const float* const* addends_host, int n_add, int64_t ld_add, float scale, double alg_bytes,
                       void* stream) {
    GD_CHECK_SHAPE(n_rows > 0 && n_virtual > 0 && d > 0 && ldx >= d && ldy >= d, "spmm: bad shape");
    GD_CHECK_ARG(n_add >= 0 && n_add <= SPMM_MAX_ADD && (n_add == 0 || (addends_host && ld_add >= d)), "spmm: bad addends");
    GD_CHECK_ARG(n_long == 0 || (lrow && lptr && partial_ws), "spmm: split rows need lrow/lptr/partial_ws");
    hipStream_t s = (hipStream_t)stream;
    SpmmAdd add;
    const bool add_al = spmm_fill_add(add, addends_host, n_add, ld_add, scale);
    GD_CHECK_ARG(n_short >= 0 && n_short <= n_virtual, "spmm: n_short out of range");
    const dim3 block(256);
    const bool vec = (d % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && gd_aligned16(X) && gd_aligned16(Y) && add_al &&
                     (partial_ws == nullptr || gd_aligned16(partial_ws));
    const int lpr = d / 4;
    const bool pow2 = vec && spmm_lpr_ok(lpr);
    if (!pow2 && n_short > 0) {
        gdmcf_set_error("spmm: the short-row path needs d in {8,16,32,64,128,256}; build the plan with n_short = 0");
        return GDMCF_E_ARG;
    }
    {
        GdProfScope prof(8, alg_bytes, s);
        if (n_short > 0) {
#define GD_SPMM_SHORT(L) hipLaunchKernelGGL(spmm_short_kernel<L>, dim3(gd_cdiv(n_short, 4 * (64 / L))), block, 0, s, vbeg, vend, vrow, n_short, col, val, X, ldx, Y, ldy, add)
            GD_SPMM_FOR_LPR(lpr, GD_SPMM_SHORT);
#undef GD_SPMM_SHORT
        }
        const int n_rest = n_virtual - n_short;
        const dim3 grid(gd_cdiv(n_rest > 0 ? n_rest : 1, 4));
        const int64_t* vbeg_r = vbeg + n_short;
        const int64_t* vend_r = vend + n_short;
        const int32_t* vrow_r = vrow + n_short;
        const int32_t* vslot_r = vslot + n_short;
#define GD_SPMM_LAUNCH(K) hipLaunchKernelGGL(K, grid, block, 0, s, vbeg_r, vend_r, vrow_r, vslot_r, n_rest, col, val, X, ldx, Y, ldy, partial_ws, d, add)
#define GD_SPMM_VEC(L) GD_SPMM_LAUNCH(spmm_vec_kernel<L>)
        if (n_rest > 0) {
            if (pow2) GD_SPMM_FOR_LPR(lpr, GD_SPMM_VEC);
            else GD_SPMM_LAUNCH(spmm_generic_kernel);
        }
#undef GD_SPMM_VEC
#undef GD_SPMM_LAUNCH
        if (n_long > 0)
            hipLaunchKernelGGL(spmm_combine_kernel, dim3(n_long), block, (size_t)4 * d * sizeof(float), s, lrow, lptr,
                               n_long, partial_ws, d, Y, ldy, add);
    }
    return gd_launch_status("spmm_csr");
}

}  // extern "C"
