// fs_incidence.h -- the unit x work incidence matrix M, shared by fs_companions.hip,
// fs_bundles.hip, fs_intervals.hip, fs_contrast.hip, fs_trends.hip and fs_saturation.hip: a unit
// (a quoted region, a scene, a character, a script word) is a row of bits over the active works,
// set where the work's coverage holds a word of the unit.  The check of the unit map, the pass
// that builds M from the kept runs, and IncJob, the host sequence around them; the coverage
// matrix of `pairs` is never built.
//
// M is stored as fs_tiles.h stores the coverage matrix, [tile of 64 units][k][64] with k over
// the 64-bit words of the active works.  Rows past n_units are zero.
//
// A call goes through IncJob as one through CoverJob: set(), the caller's own checks queued on
// the stream, number(), the caller's own refusals over a.r.n_active and mat_bytes(), reserve(),
// incidence().  inc_ksplit() is the rule by which the products over M share out its words k.
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

// The passes of one call, in this order: set(), number(), the caller's own refusals over
// a.r.n_active and mat_bytes(), reserve(), incidence().
struct IncJob {
  CoverJob cj;                  // the active flags stay in cj.flag.p
  DBuf<uint32_t> work_of, covered, bad;
  DBuf<unsigned long long> mat;

  // what every caller knows before the first pass
  static void set(IncArgs& a, uint32_t n, uint32_t n_works, uint32_t n_script,
                  uint32_t min_words, const uint32_t* d_unit_of, uint32_t n_units) {
    a.r.n = n;
    a.r.n_works = n_works;
    a.r.n_script = n_script;
    a.r.nk = (n_script + 63) / 64;
    a.r.min_words = min_words;
    a.unit_of = d_unit_of;
    a.n_units = n_units;
  }

  // The check of the unit map, which rides in front of CoverJob::number, and that: a.r numbered,
  // the sizes of M in a.m (nk, n_tiles, n_chunks, n_active = n_units).  a.r.n > 0.  The stream is
  // finished on return, after a refusal too: what the caller queued in front is there to read.
  // A bad record is refused before a bad unit map.
  int number(const fs_row* d_rows, IncArgs& a, uint32_t max_gap, hipStream_t s) {
    uint32_t bad_units = 0;
    FS_TRY(bad.reserve(1));
    FS_HIP(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    if (a.r.n_script && a.n_units)
      hipLaunchKernelGGL(k_comp_units_ok, dim3(blocks_of(a.r.n_script, kRunBlock)),
                         dim3(kRunBlock), 0, s, a.unit_of, a.r.n_script, a.n_units, bad.p);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(&bad_units, bad.p, sizeof bad_units, hipMemcpyDeviceToHost, s));
    const int rc = cj.number(d_rows, a.r, max_gap, s);
    FS_HIP(hipStreamSynchronize(s));
    if (rc != FS_OK) return rc;
    if (bad_units) {
      fs_set_error("a unit_of entry that is neither below n_units (%u) nor 0xFFFFFFFF",
                   a.n_units);
      return FS_E_INVALID;
    }
    a.m.nk = (uint32_t)(((uint64_t)a.r.n_active + 63) / 64);
    a.m.n_tiles = (uint32_t)(((uint64_t)a.n_units + kTile - 1) / kTile);
    a.m.n_chunks = (a.m.n_tiles + kChunk - 1) / kChunk;
    a.m.n_active = a.n_units;
    return FS_OK;
  }

  // the bytes of M, for the caller's own limit
  static uint64_t mat_bytes(const IncArgs& a) {
    return (uint64_t)a.m.n_tiles * kTile * a.m.nk * 8;
  }

  // The works of the active numbers (padded, FS_NONE), M (cleared) and, where the caller wants
  // works(u), the table k_pairs_covered fills: a.r.work_of, a.m.cov, a.m.covered.
  // a.r.n_active > 0; without units M is empty.
  int reserve(IncArgs& a, bool with_covered, hipStream_t s) {
    const size_t a_rows = (size_t)a.r.n_tiles * kTile;     // active numbers, padded: 64 nk
    const size_t rows = (size_t)a.m.n_tiles * kTile;
    FS_TRY(work_of.reserve(a_rows));
    FS_TRY(mat.reserve(rows * a.m.nk));
    if (with_covered) FS_TRY(covered.reserve(rows));
    FS_HIP(hipMemsetAsync(work_of.p, 0xFF, a_rows * sizeof(uint32_t), s));
    if (rows) FS_HIP(hipMemsetAsync(mat.p, 0, rows * a.m.nk * sizeof(unsigned long long), s));
    a.r.work_of = work_of.p;
    a.m.cov = mat.p;
    a.m.covered = with_covered ? covered.p : nullptr;
    return FS_OK;
  }

  // the works of the active numbers, M, works(u) where reserved (launched, not waited for)
  void incidence(const fs_row* d_rows, const IncArgs& a, hipStream_t s) {
    const dim3 blk(kRunBlock);
    hipLaunchKernelGGL(k_pairs_list, dim3(blocks_of(a.r.n_works, kRunBlock)), blk, 0, s, a.r,
                       cj.flag.p);
    if (a.n_units)
      hipLaunchKernelGGL(k_comp_incidence, dim3(blocks_of(a.r.n_runs, kRunBlock)), blk, 0, s,
                         RowsSrc{d_rows}, a, cj.flag.p);
    if (a.m.covered)
      hipLaunchKernelGGL(k_pairs_covered, dim3(a.m.n_tiles), dim3(kTile), 0, s, a.m);
  }
};

// The workgroups that share the words k of M in a product over it.  With fewer than kSplitBlocks
// workgroups in the product's own grid (`blocks` >= 1) the words are shared out until there are
// that many, at least kSplitWords words to each; the environment variable `env` sets the number
// of shares instead (for the tests).  At most nk, at least 1.
inline uint32_t inc_ksplit(const char* env, uint64_t blocks, uint32_t nk) {
  constexpr uint32_t kSplitBlocks = 512, kSplitWords = 8;
  uint32_t ksplit = env_u32(env, 0u, 65535u);
  if (!ksplit && blocks < kSplitBlocks) {
    const uint32_t room = (uint32_t)((kSplitBlocks + blocks - 1) / blocks);
    const uint32_t most = (nk + kSplitWords - 1) / kSplitWords;
    ksplit = room < most ? room : most;
  }
  if (ksplit > nk) ksplit = nk;
  return ksplit ? ksplit : 1u;
}

}  // namespace
