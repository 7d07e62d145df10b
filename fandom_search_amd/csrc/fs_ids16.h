// fs_ids16.h -- the n ids of one window out of the 16-bit copy of the fan ids (CorpusDev::tok16),
// on the host and on the device from one function (fs_ranges.h range_round; fs_debug_ids16_window).
//
// The copy holds two ids to a dword, the id at the even position in the low half.  A window at
// position p is read at the aligned position p & ~1 and shifted down by one id when p is odd:
//   d[i]  the dwords at ids + (p & ~1), ids16_dwords(n) of them
//   w[i]  = (d[i + 1] : d[i]) >> 16 * (p & 1)        one v_alignbit_b32 per pair of neighbours
//   id 2i = w[i] & 0xFFFF, id 2i + 1 = w[i] >> 16    zero-extended
// One 16-byte load holds (p & 1) + n <= 8 ids, which is every n <= 7; n = 8 at odd p needs a
// fifth dword.  An odd n takes the last id from d[n / 2] alone (the dword behind is not needed).
#ifndef FS_IDS16_H
#define FS_IDS16_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FS_IDS16_HD __host__ __device__
#else
#define FS_IDS16_HD
#endif

// dwords a window of n ids may touch from its aligned start: (1 + n) ids at odd p, rounded up
constexpr int fs_ids16_dwords(int n) { return (n + 2) / 2; }

// the low dword of (hi : lo) >> sh, sh = 0 or 16
FS_IDS16_HD inline uint32_t fs_ids16_align(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
  return (uint32_t)(((uint64_t)hi << 32 | lo) >> (sh & 31u));
#endif
}

// d[0 .. fs_ids16_dwords(N)): the dwords at the window's aligned start; odd = p & 1; f[0 .. N): the ids
template <int N>
FS_IDS16_HD inline void fs_ids16_window(const uint32_t* d, uint32_t odd, uint32_t* f) {
  static_assert(N >= 1 && N <= 8, "at most eight ids: five dwords");
  const uint32_t sh = odd << 4;
#pragma unroll
  for (int i = 0; i < (N + 1) / 2; ++i) {
    const bool last_alone = 2 * i + 1 == N;          // the window's last id, by itself in w[i]
    const uint32_t w = fs_ids16_align(last_alone ? 0u : d[i + 1], d[i], sh);
    f[2 * i] = w & 0xFFFFu;
    if (!last_alone) f[2 * i + 1] = w >> 16;
  }
}

#endif  // FS_IDS16_H
