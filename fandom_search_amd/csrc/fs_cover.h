// fs_cover.h -- the coverage row of a work, shared by fs_pairs.hip and fs_groups.hip: a bit per
// script word, set for every word a kept run spans (its first record's word to its last one's,
// bridged words included).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <hip/hip_runtime.h>

// Words o0..o1 (o0 <= o1, both inside the row) ORed into the row whose 64-bit word k is at
// row[k * stride], a 64-bit word at a time.
__device__ inline void fs_cover_span(unsigned long long* row, size_t stride, uint32_t o0,
                                     uint32_t o1) {
  const uint32_t k0 = o0 >> 6, k1 = o1 >> 6;
  for (uint32_t w = k0; w <= k1; ++w) {
    unsigned long long m = ~0ull;
    if (w == k0) m &= ~0ull << (o0 & 63);
    if (w == k1) m &= ~0ull >> (63 - (o1 & 63));
    atomicOr(&row[(size_t)w * stride], m);
  }
}
