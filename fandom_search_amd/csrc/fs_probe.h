// fs_probe.h -- the open-addressing insert fs_matches_intern (byte strings) and fs_variants
// (integer pairs) share: a table of 2^k 64-bit slots, kProbeEmpty until claimed, a slot never
// changes once claimed.  No lane ever waits on another: a lane that loses the race for a slot
// looks at what the winner wrote and goes on.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr unsigned long long kProbeEmpty = ~0ull;

// 64 well-mixed bits of x (the finalizer of splitmix64)
__host__ __device__ inline uint64_t fs_mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// The slot that holds `mine` or a word same(word) accepts as equal to it, probing linearly from
// `pos`; *inserted when this call claimed it.  The slot is read before the compare-and-swap:
// a claimed slot costs a load, which the cache serves, and only an empty one an atomic.  A stale
// "empty" only makes the swap fail, and the swap returns what is there.  The table must keep a
// free slot (callers size it to twice the keys).
template <class Same>
__device__ inline uint64_t fs_probe_insert(unsigned long long* __restrict__ slots, uint64_t mask,
                                           uint64_t pos, unsigned long long mine, Same same,
                                           bool* inserted) {
  *inserted = false;
  for (pos &= mask;; pos = (pos + 1) & mask) {
    unsigned long long cur = __hip_atomic_load(&slots[pos], __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kProbeEmpty) {
      cur = atomicCAS(&slots[pos], kProbeEmpty, mine);
      if (cur == kProbeEmpty) {
        *inserted = true;
        return pos;
      }
    }
    if (same(cur)) return pos;
  }
}

// table slots for n keys: a power of two, at least twice n (and at least 64)
inline uint64_t fs_probe_slots(uint64_t n) {
  uint64_t s = 64;
  while (s < 2 * n) s <<= 1;
  return s;
}
