// What the three SpMM generations share (spmm_csr.hip: the first; spmm_bundle.hip: the bundled and the streamed one): the fused
// addends of the LightGCN layer mean, Y = (A X + sum_k addend_k) * scale, their host-side set-up, the row epilogue that applies
// them, and the dispatch on the lanes per row.
#pragma once
#include "common.h"

namespace {

constexpr int SPMM_MAX_ADD = 8;
struct SpmmAdd {
    const float* p[SPMM_MAX_ADD];
    int n;
    int64_t ld;
    float scale;
};

// add <- (addends_host[0 .. n_add), ld_add, scale).  Returns whether the f32x4 epilogue may read the addends: every pointer
// 16-byte aligned and ld_add a multiple of 4 (true when there are none).  The caller has checked 0 <= n_add <= SPMM_MAX_ADD.
inline bool spmm_fill_add(SpmmAdd& add, const float* const* addends_host, int n_add, int64_t ld_add, float scale) {
    add = SpmmAdd{};
    add.n = n_add;
    add.ld = ld_add;
    add.scale = scale;
    bool ok = true;
    for (int k = 0; k < n_add; ++k) {
        add.p[k] = addends_host[k];
        ok = ok && gd_aligned16(add.p[k]) && (ld_add % 4 == 0);
    }
    return ok;
}

inline bool spmm_lpr_ok(int lpr) { return lpr == 2 || lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32 || lpr == 64; }

// GO(L) for the compile-time L equal to lpr = d / 4 (spmm_lpr_ok), the common widths first
#define GD_SPMM_FOR_LPR(lpr, GO)      \
    do {                              \
        if ((lpr) == 16) GO(16);      \
        else if ((lpr) == 8) GO(8);   \
        else if ((lpr) == 32) GO(32); \
        else if ((lpr) == 64) GO(64); \
        else if ((lpr) == 4) GO(4);   \
        else GO(2);                   \
    } while (0)

// Row epilogue, lane gl's 16-byte slice (columns 4 gl .. 4 gl + 3) of row r: the addends in order, then the scale, then the
// store (NT: non-temporal, for results nobody gathers from the same L2 soon).  The offsets are formed here, per use, as the
// kernels wrote them: formed at the call site they change the register allocation of spmm_short_kernel.
template <bool NT = false>
__device__ __forceinline__ void spmm_store_row(f32x4 s, const SpmmAdd& add, float* Y, int64_t ldy, int r, int gl) {
    for (int k = 0; k < add.n; ++k) s += *reinterpret_cast<const f32x4*>(add.p[k] + (int64_t)r * add.ld + gl * 4);
    if (NT) __builtin_nontemporal_store(s * add.scale, reinterpret_cast<f32x4*>(Y + (int64_t)r * ldy + gl * 4));
    else *reinterpret_cast<f32x4*>(Y + (int64_t)r * ldy + gl * 4) = s * add.scale;
}

// the same for one column (any width)
__device__ __forceinline__ void spmm_store_elem(float s, const SpmmAdd& add, float* Y, int64_t ldy, int r, int c) {
    for (int k = 0; k < add.n; ++k) s += add.p[k][(int64_t)r * add.ld + c];
    Y[(int64_t)r * ldy + c] = s * add.scale;
}

}  // namespace
