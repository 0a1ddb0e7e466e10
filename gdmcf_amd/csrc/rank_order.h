// The order every ranking kernel shares (topk.hip: the masked top-k; rank.hip: the ranks of named items): an item's key is
// the order-preserving image of its score, or of -inf when the item is masked; larger key first, equal keys in ascending item
// index -- as one 64-bit pair (key, ~index), larger pair first.  NaN, +-0 and +-inf order by their bits under this one map.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_to_float(uint32_t k) {
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

constexpr uint32_t NEG_INF_KEY = 0x007FFFFFu;  // order_key(-inf)

__device__ __forceinline__ uint32_t masked_key(const float* __restrict__ row, const uint32_t* bitmap, int i) {
    if (bitmap[i >> 5] & (1u << (i & 31))) return NEG_INF_KEY;
    return order_key(row[i]);
}

// bits of CSR row r into the LDS bitmap, as the plain kernels set their own row's (entries outside [0, I) skipped)
template <int NT>
__device__ __forceinline__ void mask_row_bits(uint32_t* bitmap, int I, const int64_t* __restrict__ indptr,
                                              const int32_t* __restrict__ indices, int64_t r, int tid) {
    const int64_t beg = indptr[r], end = indptr[r + 1];
    for (int64_t j = beg + tid; j < end; j += NT) {
        const int c = indices[j];
        if (c >= 0 && c < I) atomicOr(&bitmap[c >> 5], 1u << (c & 31));
    }
}

}  // namespace
