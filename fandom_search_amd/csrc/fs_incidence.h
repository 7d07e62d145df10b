// fs_incidence.h -- the unit x work incidence matrix M, shared by fs_companions.hip and
// fs_intervals.hip: a unit (a quoted region, a scene, a character, a script word) is a row of
// bits over the active works, set where the work's coverage holds a word of the unit.  The
// check of the unit map and the pass that builds M from the kept runs; the coverage matrix of
// `pairs` is never built.
//
// M is stored as fs_tiles.h stores the coverage matrix, [tile of 64 units][k][64] with k over
// the 64-bit words of the active works.  Rows past n_units are zero.
#pragma once
#include "fs_tiles.h"

namespace {

struct IncArgs {
  CoverArgs r;                  // the records: heads, act, work_of, n_active (cov unused)
  CoverArgs m;                  // M: cov, nk = ceil(n_active / 64), n_tiles and n_chunks of units,
                                // covered = works(u)
  const uint32_t* unit_of;      // [n_script]
  uint32_t n_units;
};

// one lane per script word
__global__ __launch_bounds__(kRunBlock) void k_comp_units_ok(const uint32_t* unit_of,
                                                             uint32_t n_script, uint32_t n_units,
                                                             uint32_t* bad_out) {
  const uint64_t o = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  bool bad = false;
  if (o < n_script) {
    const uint32_t u = unit_of[o];
    bad = u != FS_NONE && u >= n_units;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(bad_out, 1u);
}

// A lane per run (after CoverJob::number found nothing: every work and word is inside, and
// k_comp_units_ok: every unit is a row of M); the wave's kept runs are then taken in turn by
// the whole wave.
__global__ __launch_bounds__(kRunBlock) void k_comp_incidence(RowsSrc src, IncArgs a,
                                                              const uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  bool kept = false;
  uint32_t o0 = 0, o1 = 0, ai = 0;
  if (r < a.r.n_runs) {
    const uint32_t h = a.r.heads[r], e = a.r.heads[r + 1];
    if (e - h >= a.r.min_words) {
      const uint4 k = src.key(h);
      o0 = k.z;
      o1 = src.key((uint64_t)e - 1).z;                       // o0 <= o1: a run steps forward
      if (k.x < a.r.n_works && flag[k.x] && o1 < a.r.n_script && o0 <= o1) {
        kept = true;
        ai = a.r.act[k.x];
      }
    }
  }
  uint64_t todo = __ballot(kept);
  while (todo) {
    const int from = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)o0, from), b1 = (uint32_t)__shfl((int)o1, from);
    const uint32_t bi = (uint32_t)__shfl((int)ai, from);
    if (bi >= a.r.n_active) continue;                        // (never: act numbers the flagged works)
    const unsigned long long bit = 1ull << (bi & 63);
    const size_t k = bi >> 6;
    for (uint64_t o = (uint64_t)b0 + lane; o <= b1; o += 64) {
      const uint32_t u = a.unit_of[o];
      if (u >= a.n_units) continue;                          // none
      if (o != b0 && a.unit_of[o - 1] == u) continue;        // the lane at the unit's first word did it
      atomicOr(&a.m.cov[((size_t)(u / kTile) * a.m.nk + k) * kTile + u % kTile], bit);
    }
  }
}

}  // namespace
