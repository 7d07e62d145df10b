// fs_sort.h -- the sort in LDS behind the order statistics of fs_intervals.hip (k_int_stats) and
// fs_saturation.hip (k_sat_points): two arrays of P values each, P a power of two, sorted
// ascending, each on its own, by one bitonic network over the workgroup.  A caller with fewer
// than P values pads with FS_NONE, which ends up at the top.
#pragma once
#include "fs_prims.h"

// s_c and s_p ascending over P entries by a workgroup of kThreads threads; the first barrier
// stands in front of the first exchange, the last behind the last one
template <uint32_t kThreads>
__device__ inline void block_sort_two(uint32_t* s_c, uint32_t* s_p, uint32_t P) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = 2; k <= P; k <<= 1) {
    for (uint32_t j = k >> 1; j; j >>= 1) {
      __syncthreads();
      for (uint32_t i = tid; i < P; i += kThreads) {
        const uint32_t o = i ^ j;
        if (o <= i) continue;
        const bool up = (i & k) == 0;
        const uint32_t c0 = s_c[i], c1 = s_c[o], p0 = s_p[i], p1 = s_p[o];
        if ((c0 > c1) == up && c0 != c1) {
          s_c[i] = c1;
          s_c[o] = c0;
        }
        if ((p0 > p1) == up && p0 != p1) {
          s_p[i] = p1;
          s_p[o] = p0;
        }
      }
    }
  }
  __syncthreads();
}
