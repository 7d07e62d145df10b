// fs_tiles.h -- the coverage matrix of the active works and its tiled AND/popcount product,
// shared by fs_pairs.hip, fs_clusters.hip, fs_lines.hip, fs_fragments.hip and fs_digest.hip: the
// passes from the run heads to the row popcounts (CoverJob) and the 64 x 64 counts of a row tile
// against a column tile (tile_counts), of the matrix itself or of another in its layout.
//
// The matrix is stored by tiles of 64 active works, k-major: word k of row r of tile t is at
// cov[(t * nk + k) * 64 + r].  A K-slice of a tile is one contiguous piece, staged by a straight
// coalesced copy; in LDS the four adjacent rows a thread takes are 32 contiguous bytes, two
// 128-bit reads, and the lanes of a wave read 16 different such pieces (column side) or 4
// (row side, the others broadcast): no bank is asked twice.  Rows past the last active work are
// zero and share nothing.
#pragma once
#include "fs_internal.h"
#include "fs_cover.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kTile = 64;              // active works per tile (tests: TILE)
constexpr uint32_t kChunk = 8;              // column tiles a workgroup takes (tests: CHUNK)
constexpr uint32_t kSlice = 32;             // 64-bit words per K-slice (tests: K_SLICE)
constexpr uint32_t kBlock = 256;            // 16 x 16 threads, 4 x 4 pairs each
constexpr uint32_t kRunBlock = 256;
constexpr uint32_t kShStride = kTile + 1;   // of the tile of counts in LDS

// what the shared passes read and write; a command's own arguments derive from it
struct CoverArgs {
  uint32_t n, n_works, n_script, nk, n_runs, min_words, min_shared;
  uint32_t n_active, n_tiles, n_chunks;
  const uint32_t* heads;        // [n_runs + 1] first record of a run
  uint32_t* act;                // [n_works] active flag, then the active number (scanned)
  uint32_t* work_of;            // [n_tiles * 64] work of an active number (FS_NONE: padding)
  unsigned long long* cov;      // [n_tiles][nk][64] the coverage matrix
  uint32_t* covered;            // [n_tiles * 64]
  uint32_t* status;             // [0] invalid input, [1] active works
};

__global__ __launch_bounds__(kRunBlock) void k_pairs_check(RowsSrc src, CoverArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  bool bad = false;
  if (i < a.n) {
    const uint4 k = src.key(i);
    bad = k.x >= a.n_works || k.z >= a.n_script;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 1u);
}

// one lane per run (after k_pairs_check found nothing: every work and word is inside)
__global__ __launch_bounds__(kRunBlock) void k_pairs_flag(RowsSrc src, CoverArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (r >= a.n_runs) return;
  const uint32_t h = a.heads[r], e = a.heads[r + 1];
  if (e - h < a.min_words) return;
  const uint32_t w = src.key(h).x;
  if (w < a.n_works) a.act[w] = 1u;
}

// exclusive scan of in[0..nb) into out, *total = sum (one workgroup, chunks of 1024 in turn)
template <class Out>
__global__ __launch_bounds__(kScanBlock) void k_pairs_scan(const uint32_t* in, uint64_t nb,
                                                           Out* out, Out* __restrict__ total) {
  scan_array<Out, Out>(in, nb, out, total);
}

// one lane per work, before the scan's numbers replace the flags: flag[w] is kept in `flag`
__global__ __launch_bounds__(kRunBlock) void k_pairs_list(CoverArgs a, const uint32_t* flag) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w < a.n_works && flag[w]) a.work_of[a.act[w]] = (uint32_t)w;
}

__global__ __launch_bounds__(kRunBlock) void k_pairs_cover(RowsSrc src, CoverArgs a,
                                                           const uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (r >= a.n_runs) return;
  const uint32_t h = a.heads[r], e = a.heads[r + 1];
  if (e - h < a.min_words) return;
  const uint4 k = src.key(h);
  const uint32_t o0 = k.z, o1 = src.key((uint64_t)e - 1).z;     // o0 <= o1: a run steps forward
  if (k.x >= a.n_works || !flag[k.x] || o1 >= a.n_script || o0 > o1) return;
  const uint32_t ai = a.act[k.x];
  unsigned long long* row = a.cov + (size_t)(ai / kTile) * a.nk * kTile + ai % kTile;
  fs_cover_span(row, kTile, o0, o1);
}

// a workgroup of 64 lanes per tile: lane r sums row r (adjacent lanes, adjacent addresses)
// (fs_contrast.hip takes its counts from the product and does not launch it)
[[maybe_unused]] __global__ __launch_bounds__(kTile) void k_pairs_covered(CoverArgs a) {
  const unsigned long long* t = a.cov + (size_t)blockIdx.x * a.nk * kTile + threadIdx.x;
  uint32_t c = 0;
  for (uint32_t k = 0; k < a.nk; ++k) c += (uint32_t)__popcll(t[(size_t)k * kTile]);
  a.covered[(size_t)blockIdx.x * kTile + threadIdx.x] = c;
}

// The 64 x 64 counts of the row tile at ga against the column tile at gb, two tiles of nk words
// in the matrix's layout (16-byte aligned), into s_sh (stride kShStride), by a workgroup of
// kBlock threads with s_a and s_b of kSlice * kTile words each; the workgroup is synchronised on
// return.
__device__ inline void tile_counts(const unsigned long long* ga, const unsigned long long* gb,
                                   uint32_t nk, unsigned long long* s_a, unsigned long long* s_b,
                                   uint32_t* s_sh) {
  const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  uint32_t acc[4][4] = {};
  for (uint32_t k0 = 0; k0 < nk; k0 += kSlice) {
    const uint32_t kc = nk - k0 < kSlice ? nk - k0 : kSlice;
    const ulonglong2* va = reinterpret_cast<const ulonglong2*>(ga + (size_t)k0 * kTile);
    const ulonglong2* vb = reinterpret_cast<const ulonglong2*>(gb + (size_t)k0 * kTile);
    for (uint32_t v = threadIdx.x; v < kc * (kTile / 2); v += kBlock) {
      reinterpret_cast<ulonglong2*>(s_a)[v] = va[v];
      reinterpret_cast<ulonglong2*>(s_b)[v] = vb[v];
    }
    __syncthreads();
    for (uint32_t k = 0; k < kc; ++k) {
      const ulonglong2* pa = reinterpret_cast<const ulonglong2*>(s_a + k * kTile + ty * 4);
      const ulonglong2* pb = reinterpret_cast<const ulonglong2*>(s_b + k * kTile + tx * 4);
      const ulonglong2 a01 = pa[0], a23 = pa[1], b01 = pb[0], b23 = pb[1];
      const unsigned long long ra[4] = {a01.x, a01.y, a23.x, a23.y};
      const unsigned long long rb[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) acc[i][j] += (uint32_t)__popcll(ra[i] & rb[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i)
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) s_sh[(ty * 4 + i) * kShStride + tx * 4 + j] = acc[i][j];
  __syncthreads();
}

// the same for row tile ti against column tile tj of the coverage matrix
__device__ inline void tile_counts(const CoverArgs& a, uint32_t ti, uint32_t tj,
                                   unsigned long long* s_a, unsigned long long* s_b,
                                   uint32_t* s_sh) {
  tile_counts(a.cov + (size_t)ti * a.nk * kTile, a.cov + (size_t)tj * a.nk * kTile, a.nk, s_a,
              s_b, s_sh);
}

// What two rows of the matrix share (k_pairs_detail, k_tree_detail): the AND of the rows at ra
// and rb, nk words kTile apart, walked a 64-bit word at a time, the open run's start and length
// carried from word to word.  The number of shared words, the smallest (FS_NONE without one) and
// the largest of them, and the start and length of their longest run, the first among equals.
struct SharedRun {
  uint32_t shared, first, last, run_first, run_words;
};

__device__ inline SharedRun shared_run(const unsigned long long* ra, const unsigned long long* rb,
                                       uint32_t nk) {
  uint32_t shared = 0, first = FS_NONE, last = 0, best_s = 0, best_n = 0, cur_s = 0, cur_n = 0;
  for (uint32_t k = 0; k < nk; ++k) {
    unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    const uint32_t base = k * 64;
    if (x == 0) {
      if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
      cur_n = 0;
      continue;
    }
    shared += (uint32_t)__popcll(x);
    if (first == FS_NONE) first = base + (uint32_t)__builtin_ctzll(x);
    last = base + 63 - (uint32_t)__builtin_clzll(x);
    if (x == ~0ull) {
      if (!cur_n) cur_s = base;
      cur_n += 64;
      continue;
    }
    const uint32_t t = (uint32_t)__builtin_ctzll(~x);      // ones from bit 0 on: the open run goes on
    if (t) {
      if (!cur_n) cur_s = base;
      cur_n += t;
      x &= ~0ull << t;
    }
    if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
    cur_n = 0;
    while (x) {
      const uint32_t s = (uint32_t)__builtin_ctzll(x);     // s >= 1: bit t is clear
      const uint32_t l = (uint32_t)__builtin_ctzll(~(x >> s));
      if (s + l == 64) {                                   // up to the word's last bit: left open
        cur_s = base + s;
        cur_n = l;
        break;
      }
      if (l > best_n) { best_n = l; best_s = base + s; }
      x &= ~0ull << (s + l);
    }
  }
  if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
  return SharedRun{shared, first, last, best_s, best_n};
}

// The shared passes of one call, in this order: number(), the caller's own refusals over
// a.n_active, reserve(), cover().
struct CoverJob {
  DBuf<uint32_t> flag, act, work_of, covered, status;
  DBuf<unsigned long long> cov;
  fs_runs* runs = nullptr;
  ~CoverJob() {
    if (runs) fs_runs_free(runs);
  }

  // Run heads, the check of every record, the active works numbered in work order: a.heads,
  // a.n_runs, a.act (the numbers; the flags stay in flag.p), a.status, a.n_active, a.n_tiles
  // and a.n_chunks set.  a.n, a.n_works, a.n_script, a.nk and a.min_words are the caller's;
  // a.n > 0.  Finished on return.
  int number(const fs_row* d_rows, CoverArgs& a, uint32_t max_gap, hipStream_t s) {
    FS_TRY(fs_runs_find(d_rows, a.n, a.min_words, max_gap, s, &runs, &a.heads, &a.n_runs));
    if (!a.n_works || !a.n_script) return invalid();
    FS_TRY(flag.reserve(a.n_works));
    FS_TRY(act.reserve(a.n_works));
    FS_TRY(status.reserve(4));
    FS_HIP(hipMemsetAsync(flag.p, 0, (size_t)a.n_works * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(status.p, 0, 4 * sizeof(uint32_t), s));
    a.act = flag.p;                                  // k_pairs_flag writes the flags
    a.status = status.p;
    const RowsSrc src{d_rows};
    const dim3 blk(kRunBlock);
    hipLaunchKernelGGL(k_pairs_check, dim3((a.n + kRunBlock - 1) / kRunBlock), blk, 0, s, src, a);
    hipLaunchKernelGGL(k_pairs_flag, dim3((a.n_runs + kRunBlock - 1) / kRunBlock), blk, 0, s, src,
                       a);
    hipLaunchKernelGGL(k_pairs_scan<uint32_t>, dim3(1), dim3(kScanBlock), 0, s, flag.p,
                       (uint64_t)a.n_works, act.p, status.p + 1);
    FS_HIP(hipGetLastError());
    uint32_t st[2];
    FS_HIP(hipMemcpyAsync(st, status.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (st[0]) return invalid();
    a.act = act.p;
    a.n_active = st[1];
    a.n_tiles = (a.n_active + kTile - 1) / kTile;
    a.n_chunks = (a.n_tiles + kChunk - 1) / kChunk;
    return FS_OK;
  }

  // the matrix and its per-row tables, cleared (a.n_active > 0)
  int reserve(CoverArgs& a, hipStream_t s) {
    const size_t rows = (size_t)a.n_tiles * kTile;
    FS_TRY(work_of.reserve(rows));
    FS_TRY(covered.reserve(rows));
    FS_TRY(cov.reserve(rows * a.nk));
    FS_HIP(hipMemsetAsync(work_of.p, 0xFF, rows * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(cov.p, 0, rows * a.nk * sizeof(unsigned long long), s));
    a.work_of = work_of.p;
    a.covered = covered.p;
    a.cov = cov.p;
    return FS_OK;
  }

  // the works of the active numbers, the matrix, the row popcounts (launched, not waited for)
  void cover(const fs_row* d_rows, const CoverArgs& a, hipStream_t s) {
    const dim3 blk(kRunBlock);
    hipLaunchKernelGGL(k_pairs_list, dim3((a.n_works + kRunBlock - 1) / kRunBlock), blk, 0, s, a,
                       flag.p);
    hipLaunchKernelGGL(k_pairs_cover, dim3((a.n_runs + kRunBlock - 1) / kRunBlock), blk, 0, s,
                       RowsSrc{d_rows}, a, flag.p);
    hipLaunchKernelGGL(k_pairs_covered, dim3(a.n_tiles), dim3(kTile), 0, s, a);
  }

  static int invalid() {
    fs_set_error("a work >= n_works or an orig_ix >= n_script");
    return FS_E_INVALID;
  }
};

}  // namespace
