// fs_bundles.hip -- `ao3.py bundles`: sets of stretches of the script that the same fan works
// quote (fs_bundles, fs_bundles_rows in include/fandom_search.h).  `companions` relates the
// units two at a time; this unit mines every set of 2 .. max_size units that at least min_all
// active works quote in full, level by level over the rows of the incidence matrix M of
// fs_incidence.h, and one level more, which says of every listed set whether it is closed and
// how many frequent sets extend it.
//
// Every output is an integer count, a minimum or an OR, and every place comes from a scanned
// count, so no schedule changes a byte.  Separate launches on one stream; no workgroup waits
// on another:
//   incidence        IncJob of fs_incidence.h: M and works(u), then
//   k_bun_rows       the unit-major copy of M, [unit][nkp] with nkp = ceil(N / 64) rounded up to
//                    four words: the count pass reads the rows of arbitrary units, and the tiled
//                    layout keeps a row's words 512 bytes apart
//   k_bun_tiles<0>   level 2: tile_counts over M with the keep rule both >= min_all
//   k_pairs_scan     offsets in (row, chunk) order: F_2 comes out in (a, b) order, no sort
//   k_bun_tiles<1>   the pairs placed
//  per level k -> k + 1:
//   k_bun_join       a lane per set of F_k: the end of its prefix group by binary search (the
//                    list is sorted), its candidates and its work items of kPiece extensions
//   k_pairs_scan     the offsets of both and the level's totals, which the host reads
//   k_bun_cands      a lane per candidate: its parent, and (FS_BUNDLES_PRUNE) whether one of
//                    its other k-subsets is missing from F_k
//   k_bun_count      the hot pass, a workgroup per work item: the AND of the parent's k rows is
//                    built once per K-slice of kBunSlice words in LDS, every thread a word;
//                    each wave then takes extensions of the piece in turn, a lane reading four
//                    adjacent words of the extension's row (two 16-byte loads, a wave one
//                    contiguous KiB) against the slice, the popcounts summed over the wave
//   k_pairs_scan     the kept candidates numbered in candidate order: F_k+1 is sorted
//   k_bun_place      the kept candidates written as the next level
//   k_bun_first      a lane per set: the AND of its rows from the front to its first set bit
//   k_bun_mark       a lane per (set of F_k+1, unit left out): the k-subset found in F_k by
//                    binary search, its extensions counted, closed cleared on equal works
//  then
//   k_bun_tally      a lane per set of 2 .. max_size units: sets and largest of its units, the
//                    closed and the maximal sets of its level
//   k_bun_emit       the fs_bundle records
#include "fs_incidence.h"

namespace {

constexpr uint32_t kBunSlice = kBlock;      // 64-bit words of a K-slice: one per thread
constexpr uint32_t kBunPerWave = 16;        // extensions a wave takes
constexpr uint32_t kBunPiece = 4 * kBunPerWave;   // extensions of a work item (tests: PIECE)
constexpr uint32_t kMaxSize = FS_BUNDLES_MAX_SIZE;

// F_k: n sets of k units each
struct BunLevel {
  uint32_t* items;              // [n][k] ascending
  uint32_t* works;              // [n]
  uint32_t* first;              // [n] active number of the first work quoting all of it
  uint32_t* ext;                // [n] frequent sets of k + 1 units that hold it
  uint32_t* closed;             // [n]
  uint32_t n, k;
};

struct BunArgs : IncArgs {      // r, m, unit_of, n_units: fs_incidence.h
  uint32_t min_all;
  const unsigned long long* rows;   // [n_units][nkp]
  uint32_t nkp;
  uint32_t* cnt;                // [m.n_tiles * 64][n_chunks] kept pairs of a row in a chunk
  unsigned long long* off;      // the same, scanned
  uint32_t* any;                // [m.n_tiles][n_chunks] bit t: column tile t of the chunk keeps a pair
  BunLevel f2;
};

// one lane per word of the copy
__global__ __launch_bounds__(kRunBlock) void k_bun_rows(BunArgs a, unsigned long long* rows) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= (uint64_t)a.n_units * a.nkp) return;
  const uint32_t u = (uint32_t)(i / a.nkp), k = (uint32_t)(i % a.nkp);
  rows[i] = k < a.m.nk ? a.m.cov[((size_t)(u / kTile) * a.m.nk + k) * kTile + u % kTile] : 0ull;
}

// one lane per unit: the units with works(u) >= min_all, whose pairs are level 2's candidates
__global__ __launch_bounds__(kRunBlock) void k_bun_singles(BunArgs a, uint32_t* n_out) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint64_t m = __ballot(u < a.n_units && a.m.covered[u] >= a.min_all);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(n_out, (uint32_t)__popcll(m));
}

// blockIdx.x = row tile * n_chunks + chunk.  kPlace 0: the counts; 1: the pairs.
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_bun_tiles(BunArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ uint32_t s_rowcnt[kTile];
  __shared__ unsigned long long s_cur[kTile];
  __shared__ uint32_t s_any;
  const uint32_t n_chunks = a.m.n_chunks, n_tiles = a.m.n_tiles;
  const uint32_t ti = blockIdx.x / n_chunks, c = blockIdx.x % n_chunks;
  const uint32_t tj0 = ti > c * kChunk ? ti : c * kChunk;
  const uint32_t tj1 = (c + 1) * kChunk < n_tiles ? (c + 1) * kChunk : n_tiles;
  if (tj0 >= tj1) return;                                // below the diagonal
  const uint32_t mask = kPlace ? a.any[blockIdx.x] : 0u;
  if (kPlace && !mask) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kTile) {
    s_rowcnt[threadIdx.x] = 0;
    if (kPlace) s_cur[threadIdx.x] = a.off[((size_t)ti * kTile + threadIdx.x) * n_chunks + c];
  }
  if (threadIdx.x == 0) s_any = 0;
  for (uint32_t tj = tj0; tj < tj1; ++tj) {
    if (kPlace && !((mask >> (tj - c * kChunk)) & 1)) continue;
    __syncthreads();                                     // s_sh of the tile before
    tile_counts(a.m, ti, tj, s_a, s_b, s_sh);
    const bool diag = tj == ti;
    // wave w takes rows 16 w .. 16 w + 15, a lane per column
    bool kept_any = false;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const bool keep = sh >= a.min_all && (!diag || r < lane);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      kept_any = true;
      if (kPlace) {
        const unsigned long long pos = s_cur[r] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (keep) {
          reinterpret_cast<uint2*>(a.f2.items)[pos] = make_uint2(ti * kTile + r, tj * kTile + lane);
          a.f2.works[pos] = sh;
          a.f2.ext[pos] = 0u;
          a.f2.closed[pos] = 1u;
        }
        if (lane == 0) s_cur[r] += (uint32_t)__popcll(m);
      } else if (lane == 0) {
        s_rowcnt[r] += (uint32_t)__popcll(m);
      }
    }
    if (!kPlace && kept_any && lane == 0) atomicOr(&s_any, 1u << (tj - c * kChunk));
  }
  if (kPlace) return;
  __syncthreads();
  if (threadIdx.x < kTile)
    a.cnt[((size_t)ti * kTile + threadIdx.x) * n_chunks + c] = s_rowcnt[threadIdx.x];
  if (threadIdx.x == 0) a.any[blockIdx.x] = s_any;
}

// the first k units of set x of `f` against key: -1, 0, 1
__device__ inline int bun_cmp(const BunLevel& f, uint64_t x, const uint32_t* key, uint32_t k) {
  const uint32_t* it = f.items + x * f.k;
  for (uint32_t t = 0; t < k; ++t) {
    if (it[t] != key[t]) return it[t] < key[t] ? -1 : 1;
  }
  return 0;
}

// the place of the set `key` (f.k units) in f, f.n without it
__device__ inline uint32_t bun_find(const BunLevel& f, const uint32_t* key) {
  uint32_t lo = 0, hi = f.n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bun_cmp(f, mid, key, f.k) < 0) lo = mid + 1; else hi = mid;
  }
  return lo < f.n && bun_cmp(f, lo, key, f.k) == 0 ? lo : f.n;
}

// One lane per set i of F_k: the sets behind it that share its first k - 1 units are its
// extensions; n_cand[i] of them, in n_item[i] pieces of kBunPiece.
__global__ __launch_bounds__(kRunBlock) void k_bun_join(BunLevel f, uint32_t* n_cand,
                                                        uint32_t* n_item) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= f.n) return;
  uint32_t key[kMaxSize + 1];
  for (uint32_t t = 0; t + 1 < f.k; ++t) key[t] = f.items[i * f.k + t];
  uint32_t lo = (uint32_t)i + 1, hi = f.n;               // first set past the group
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (bun_cmp(f, mid, key, f.k - 1) == 0) lo = mid + 1; else hi = mid;
  }
  const uint32_t n = lo - (uint32_t)i - 1;
  n_cand[i] = n;
  n_item[i] = (n + kBunPiece - 1) / kBunPiece;
}

// the largest i < n with off[i] <= x, off ascending with off[0] = 0 and x < off[n]
__device__ inline uint32_t bun_owner(const unsigned long long* off, uint32_t n,
                                     unsigned long long x) {
  uint32_t lo = 0, hi = n;                               // off[lo] <= x < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// One lane per candidate c = F_k[i] + the last unit of F_k[j]: parent[c] = i; dead[c] = 1 when
// `prune` and a k-subset other than F_k[i] and F_k[j] is missing from F_k.
__global__ __launch_bounds__(kRunBlock) void k_bun_cands(BunLevel f, const unsigned long long* off,
                                                         uint64_t n_cands, uint32_t prune,
                                                         uint32_t* parent, uint32_t* dead) {
  const uint64_t c = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (c >= n_cands) return;
  const uint32_t i = bun_owner(off, f.n, c);
  parent[c] = i;
  uint32_t gone = 0;
  if (prune && f.k >= 2) {
    const uint32_t j = i + 1 + (uint32_t)(c - off[i]);
    uint32_t all[kMaxSize + 1], key[kMaxSize + 1];
    for (uint32_t t = 0; t < f.k; ++t) all[t] = f.items[(uint64_t)i * f.k + t];
    all[f.k] = f.items[(uint64_t)j * f.k + f.k - 1];
    for (uint32_t out = 0; out + 1 < f.k && !gone; ++out) {   // a unit of the shared prefix left out
      for (uint32_t t = 0, w = 0; t <= f.k; ++t)
        if (t != out) key[w++] = all[t];
      gone = bun_find(f, key) == f.n;
    }
  }
  dead[c] = gone;
}

// blockIdx.x = a work item: piece p of the extensions of parent i.
__global__ __launch_bounds__(kBlock) void k_bun_count(BunArgs a, BunLevel f,
                                                      const unsigned long long* cand_off,
                                                      const unsigned long long* item_off,
                                                      const uint32_t* dead, uint32_t* count,
                                                      uint32_t* keep) {
  __shared__ __align__(16) unsigned long long s_and[kBunSlice];
  __shared__ uint32_t s_unit[kMaxSize];
  __shared__ uint32_t s_ext[kBunPiece];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = bun_owner(item_off, f.n, blockIdx.x);
  const unsigned long long c0 = cand_off[i];
  const uint32_t n_ext = (uint32_t)(cand_off[i + 1] - c0);
  const uint32_t e0 = (uint32_t)(blockIdx.x - item_off[i]) * kBunPiece;
  if (threadIdx.x < f.k) s_unit[threadIdx.x] = f.items[(uint64_t)i * f.k + threadIdx.x];
  if (threadIdx.x < kBunPiece) {
    const uint32_t e = e0 + threadIdx.x;
    uint32_t x = FS_NONE;
    if (e < n_ext && !dead[c0 + e]) x = f.items[((uint64_t)i + 1 + e) * f.k + f.k - 1];
    s_ext[threadIdx.x] = x;
  }
  uint32_t acc[kBunPerWave] = {};
  const uint32_t nkp = a.nkp;
  for (uint32_t k0 = 0; k0 < nkp; k0 += kBunSlice) {
    __syncthreads();                                     // s_unit, s_ext; s_and of the slice before
    const uint32_t w = k0 + threadIdx.x;
    unsigned long long v = 0ull;
    if (w < nkp) {
      v = ~0ull;
      for (uint32_t t = 0; t < f.k; ++t) v &= a.rows[(size_t)s_unit[t] * nkp + w];
    }
    s_and[threadIdx.x] = v;
    __syncthreads();
    const uint32_t w4 = k0 + lane * 4;                   // nkp is a multiple of 4
    if (w4 >= nkp) continue;
    const ulonglong2 p01 = reinterpret_cast<const ulonglong2*>(s_and)[lane * 2];
    const ulonglong2 p23 = reinterpret_cast<const ulonglong2*>(s_and)[lane * 2 + 1];
    if (!(p01.x | p01.y | p23.x | p23.y)) continue;
#pragma unroll
    for (uint32_t t = 0; t < kBunPerWave; ++t) {
      const uint32_t x = s_ext[wave * kBunPerWave + t];
      if (x == FS_NONE) continue;
      const ulonglong2* row = reinterpret_cast<const ulonglong2*>(a.rows + (size_t)x * nkp + w4);
      const ulonglong2 r01 = row[0], r23 = row[1];
      acc[t] += (uint32_t)(__popcll(p01.x & r01.x) + __popcll(p01.y & r01.y) +
                           __popcll(p23.x & r23.x) + __popcll(p23.y & r23.y));
    }
  }
#pragma unroll
  for (uint32_t t = 0; t < kBunPerWave; ++t) {
    const uint32_t e = e0 + wave * kBunPerWave + t;
    if (e >= n_ext) break;                               // (wave-uniform)
    const uint32_t n = wave_sum(acc[t]);
    if (lane == 0) {
      count[c0 + e] = n;
      keep[c0 + e] = n >= a.min_all ? 1u : 0u;
    }
  }
}

// one lane per candidate: a kept one becomes set pos[c] of F_k+1
__global__ __launch_bounds__(kRunBlock) void k_bun_place(BunLevel f, BunLevel g,
                                                         const unsigned long long* cand_off,
                                                         uint64_t n_cands, const uint32_t* parent,
                                                         const uint32_t* count,
                                                         const uint32_t* keep,
                                                         const uint32_t* pos) {
  const uint64_t c = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (c >= n_cands || !keep[c]) return;
  const uint32_t i = parent[c], j = i + 1 + (uint32_t)(c - cand_off[i]);
  const uint64_t p = pos[c];
  for (uint32_t t = 0; t < f.k; ++t) g.items[p * g.k + t] = f.items[(uint64_t)i * f.k + t];
  g.items[p * g.k + f.k] = f.items[(uint64_t)j * f.k + f.k - 1];
  g.works[p] = count[c];
  g.ext[p] = 0u;
  g.closed[p] = 1u;
}

// One lane per set: the AND of its rows from the front up to its first set bit.  A frequent
// set has works >= 1, so it is found.
__global__ __launch_bounds__(kRunBlock) void k_bun_first(BunArgs a, BunLevel f) {
  const uint64_t s = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (s >= f.n) return;
  uint32_t u[kMaxSize + 1];
  for (uint32_t t = 0; t < f.k; ++t) u[t] = f.items[s * f.k + t];
  uint32_t first = FS_NONE;
  for (uint32_t k = 0; k < a.m.nk; ++k) {
    unsigned long long x = ~0ull;
    for (uint32_t t = 0; t < f.k; ++t) x &= a.rows[(size_t)u[t] * a.nkp + k];
    if (x) {
      first = k * 64 + (uint32_t)__builtin_ctzll(x);
      break;
    }
  }
  f.first[s] = first;
}

// one lane per (set of g = F_k+1, unit left out)
__global__ __launch_bounds__(kRunBlock) void k_bun_mark(BunLevel f, BunLevel g) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= (uint64_t)g.n * g.k) return;
  const uint64_t s = i / g.k;
  const uint32_t out = (uint32_t)(i % g.k);
  uint32_t key[kMaxSize + 1];
  for (uint32_t t = 0, w = 0; t < g.k; ++t)
    if (t != out) key[w++] = g.items[s * g.k + t];
  const uint32_t at = bun_find(f, key);
  if (at == f.n) return;                                 // (never: every subset is frequent)
  atomicAdd(&f.ext[at], 1u);
  if (f.works[at] == g.works[s]) f.closed[at] = 0u;      // (every writer writes 0)
}

// one lane per set of a listed level: stats[0] closed, stats[1] maximal sets of the level
__global__ __launch_bounds__(kRunBlock) void k_bun_tally(BunLevel f, fs_bundle_unit* units,
                                                         uint32_t* stats) {
  const uint64_t s = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const bool in = s < f.n;
  if (in) {
    for (uint32_t t = 0; t < f.k; ++t) {
      fs_bundle_unit* u = units + f.items[s * f.k + t];
      atomicAdd(&u->sets, 1u);
      atomicMax(&u->largest, f.k);
    }
  }
  const uint64_t mc = __ballot(in && f.closed[s]), mm = __ballot(in && !f.ext[s]);
  if ((threadIdx.x & 63) == 0) {
    if (mc) atomicAdd(&stats[0], (uint32_t)__popcll(mc));
    if (mm) atomicAdd(&stats[1], (uint32_t)__popcll(mm));
  }
}

// one lane per unit
__global__ __launch_bounds__(kRunBlock) void k_bun_units(const uint32_t* covered,
                                                         fs_bundle_unit* units,
                                                         uint32_t n_units) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u < n_units)
    reinterpret_cast<uint4*>(units)[u] = make_uint4(covered ? covered[u] : 0u, 0u, 0u, 0u);
}

// one lane per set: record base + s
__global__ __launch_bounds__(kRunBlock) void k_bun_emit(BunLevel f, const uint32_t* work_of,
                                                        uint32_t n_active, fs_bundle* out,
                                                        uint64_t base) {
  const uint64_t s = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (s >= f.n) return;
  uint32_t u[kMaxSize];
  for (uint32_t t = 0; t < kMaxSize; ++t) u[t] = t < f.k ? f.items[s * f.k + t] : FS_NONE;
  const uint32_t fa = f.first[s];
  uint4* o = reinterpret_cast<uint4*>(out + base + s);
  o[0] = make_uint4(u[0], u[1], u[2], u[3]);
  o[1] = make_uint4(u[4], u[5], u[6], u[7]);
  o[2] = make_uint4(f.k, f.works[s], fa < n_active ? work_of[fa] : FS_NONE, f.ext[s]);
  o[3] = make_uint4(f.closed[s], 0u, 0u, 0u);
}

constexpr int kTimes = FS_BUNDLES_TIMES;
thread_local double t_ms[kTimes];   // fs_bundles_times in include/fandom_search.h

struct LevelBufs {
  DBuf<uint32_t> items, works, first, ext, closed;
  int reserve(uint64_t n, uint32_t k) {
    FS_TRY(items.reserve(n * k));
    FS_TRY(works.reserve(n));
    FS_TRY(first.reserve(n));
    FS_TRY(ext.reserve(n));
    FS_TRY(closed.reserve(n));
    return FS_OK;
  }
  BunLevel view(uint64_t n, uint32_t k) {
    return BunLevel{items.p, works.p, first.p, ext.p, closed.p, (uint32_t)n, k};
  }
};

// one call: mine() through the units, the levels and the number of sets, then write()
struct BunJob {
  IncJob inc;
  DBuf<uint32_t> cnt, any, n_cand, n_item, parent, dead, count, keep, pos, stats;
  DBuf<unsigned long long> rows, off, cand_off, item_off, totals;
  DBuf<fs_bundle_unit> units;       // the caller's are written when nothing can refuse any more
  LevelBufs lv[kMaxSize + 2];       // by size
  BunLevel f[kMaxSize + 2] = {};
  Clock<48> clk;
  BunArgs a{};
  uint32_t max_size = 0;
  uint64_t n_sets = 0, max_sets = 0, bytes = 0, scratch = 0;
  fs_bundle_level levels[kMaxSize] = {};     // sizes 2 .. max_size + 1

  void blank_levels() {
    for (uint32_t s = 2; s <= max_size + 1; ++s) {
      const uint32_t none = s > max_size ? FS_NONE : 0u;
      levels[s - 2] = fs_bundle_level{s, 0u, 0ull, none, none};
    }
  }

  int none(fs_bundle_unit* d_units, hipStream_t s) {
    if (a.n_units)
      hipLaunchKernelGGL(k_bun_units, dim3(blocks_of(a.n_units, kRunBlock)), dim3(kRunBlock), 0,
                         s, (const uint32_t*)nullptr, d_units, a.n_units);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }

  // what the tables of a call hold, against FS_BUNDLES_MAX_BYTES
  // (`more` stays for the call, `now` is scratch that the next level uses again)
  int room(uint64_t more, uint64_t now, uint32_t size, const char* what) {
    bytes += more;
    if (now > scratch) scratch = now;
    if (bytes + scratch > FS_BUNDLES_MAX_BYTES) {
      fs_set_error("bundles: the incidence matrix twice, the level lists and the candidate "
                   "buffers come to more than %u bytes at %s of size %u; raise --min-all or "
                   "lower --max-size", FS_BUNDLES_MAX_BYTES, what, size);
      return FS_E_UNSUPPORTED;
    }
    return FS_OK;
  }

  int too_many(uint32_t size, unsigned long long n) {
    fs_set_error("bundles: level %u has %llu candidate sets, more than %llu "
                 "(FS_BUNDLES_MAX_SETS); raise --min-all or lower --max-size", size, n,
                 (unsigned long long)max_sets);
    return FS_E_UNSUPPORTED;
  }

  // d_units written, levels and n_sets set (all on `s`, finished on return)
  int mine(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
           const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
           uint32_t min_all, uint32_t k_max, fs_bundle_unit* d_units, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    max_size = k_max;
    blank_levels();
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.min_all = min_all;
    if (!n || !n_units) return none(d_units, s);
    max_sets = env_u32("FS_BUNDLES_MAX_SETS", FS_BUNDLES_MAX_SETS, 1u << 26);
    const uint32_t prune = env_u32("FS_BUNDLES_PRUNE", 1u, 1u);
    FS_TRY(inc.number(d_rows, a, max_gap, s));
    if (!a.r.n_active) return none(d_units, s);
    const uint64_t nkp = ((uint64_t)a.m.nk + 3) / 4 * 4;
    bytes = IncJob::mat_bytes(a) + (uint64_t)n_units * nkp * 8;
    if (bytes > FS_BUNDLES_MAX_BYTES) {
      fs_set_error("%u units over %u works with a passage: the incidence matrix and its "
                   "unit-major copy come to more than %u bytes", n_units, a.r.n_active,
                   FS_BUNDLES_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    a.nkp = (uint32_t)nkp;
    const size_t rows_n = (size_t)a.m.n_tiles * kTile, cells = rows_n * a.m.n_chunks;
    const uint64_t blocks = (uint64_t)a.m.n_tiles * a.m.n_chunks;
    if (blocks > 0x7FFFFFFFull || (uint64_t)n_units * nkp > 0x7FFFFFFFull * kRunBlock) {
      fs_set_error("%u units: more tiles of pairs than a launch takes", n_units);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(inc.reserve(a, true, s));
    FS_TRY(rows.reserve((size_t)n_units * nkp));
    FS_TRY(cnt.reserve(cells));
    FS_TRY(off.reserve(cells));
    FS_TRY(any.reserve((size_t)blocks));
    FS_TRY(totals.reserve(2));
    FS_TRY(stats.reserve(2 * (kMaxSize + 2)));
    FS_TRY(units.reserve(n_units));
    FS_HIP(hipMemsetAsync(cnt.p, 0, cells * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(any.p, 0, (size_t)blocks * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(stats.p, 0, 2 * (kMaxSize + 2) * sizeof(uint32_t), s));
    a.rows = rows.p;
    a.cnt = cnt.p;
    a.off = off.p;
    a.any = any.p;
    const dim3 blk(kRunBlock);
    FS_TRY(clk.mark(0, s));
    inc.incidence(d_rows, a, s);
    hipLaunchKernelGGL(k_bun_rows, dim3(blocks_of((uint64_t)n_units * nkp, kRunBlock)), blk, 0,
                       s, a, rows.p);
    hipLaunchKernelGGL(k_bun_units, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s,
                       (const uint32_t*)a.m.covered, units.p, n_units);
    FS_TRY(clk.mark(1, s));
    // level 2: stats[0] is borrowed for the number of units with works >= min_all
    hipLaunchKernelGGL(k_bun_singles, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s, a,
                       stats.p);
    hipLaunchKernelGGL(k_bun_tiles<0>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s, cnt.p,
                       (uint64_t)cells, off.p, totals.p);
    FS_HIP(hipGetLastError());
    unsigned long long tot[2] = {0, 0};
    uint32_t singles = 0;
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot[0], hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(&singles, stats.p, sizeof singles, hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemsetAsync(stats.p, 0, sizeof(uint32_t), s));
    FS_HIP(hipStreamSynchronize(s));
    levels[0].candidates = (uint64_t)singles * (singles ? singles - 1 : 0) / 2;
    if (tot[0] > max_sets) return too_many(2, tot[0]);
    FS_TRY(room(tot[0] * (2 + 4) * 4, 0, 2, "the list"));
    FS_TRY(lv[2].reserve(tot[0], 2));
    f[2] = lv[2].view(tot[0], 2);
    levels[0].frequent = (uint32_t)tot[0];
    if (f[2].n) {
      a.f2 = f[2];
      hipLaunchKernelGGL(k_bun_tiles<1>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
      hipLaunchKernelGGL(k_bun_first, dim3(blocks_of(f[2].n, kRunBlock)), blk, 0, s, a, f[2]);
    }
    FS_TRY(clk.mark(2, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    for (uint32_t k = 2; k <= max_size; ++k) FS_TRY(level(k, prune, s));
    FS_TRY(clk.mark(3, s));
    for (uint32_t k = 2; k <= max_size; ++k) {
      if (!f[k].n) continue;
      hipLaunchKernelGGL(k_bun_tally, dim3(blocks_of(f[k].n, kRunBlock)), blk, 0, s, f[k],
                         units.p, stats.p + 2 * k);
      n_sets += f[k].n;
    }
    FS_TRY(clk.mark(4, s));
    FS_HIP(hipGetLastError());
    uint32_t st[2 * (kMaxSize + 2)];
    FS_HIP(hipMemcpyAsync(st, stats.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(d_units, units.p, (size_t)n_units * sizeof(fs_bundle_unit),
                          hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    for (uint32_t k = 2; k <= max_size; ++k) {
      levels[k - 2].closed = st[2 * k];
      levels[k - 2].maximal = st[2 * k + 1];
    }
    t_ms[kTimes - 2] = clk.elapsed(3, 4);
    return FS_OK;
  }

  // F_k+1 from F_k, and what it says about F_k
  int level(uint32_t k, uint32_t prune, hipStream_t s) {
    const uint32_t n = f[k].n;
    f[k + 1] = BunLevel{nullptr, nullptr, nullptr, nullptr, nullptr, 0u, k + 1};
    if (n < 2) return FS_OK;
    const dim3 blk(kRunBlock);
    const int m0 = 5 + (int)(k - 2) * 5;                  // marks of this level
    double* t = t_ms + 2 + (k - 2) * 4;
    FS_TRY(room(0, (uint64_t)n * 24, k + 1, "the join"));
    FS_TRY(n_cand.reserve(n));
    FS_TRY(n_item.reserve(n));
    FS_TRY(cand_off.reserve((size_t)n + 1));
    FS_TRY(item_off.reserve((size_t)n + 1));
    FS_TRY(clk.mark(m0, s));
    hipLaunchKernelGGL(k_bun_join, dim3(blocks_of(n, kRunBlock)), blk, 0, s, f[k], n_cand.p,
                       n_item.p);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s,
                       n_cand.p, (uint64_t)n, cand_off.p, totals.p);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s,
                       n_item.p, (uint64_t)n, item_off.p, totals.p + 1);
    FS_HIP(hipGetLastError());
    unsigned long long tot[2] = {0, 0};
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot, hipMemcpyDeviceToHost, s));
    // the scans leave off[n] to the totals: the owner searches read it
    FS_HIP(hipMemcpyAsync(cand_off.p + n, totals.p, sizeof tot[0], hipMemcpyDeviceToDevice, s));
    FS_HIP(hipMemcpyAsync(item_off.p + n, totals.p + 1, sizeof tot[0], hipMemcpyDeviceToDevice,
                          s));
    FS_HIP(hipStreamSynchronize(s));
    levels[k - 1].candidates = tot[0];
    if (tot[0] > max_sets) return too_many(k + 1, tot[0]);
    if (!tot[0]) return FS_OK;
    FS_TRY(room(0, (uint64_t)n * 24 + tot[0] * 20, k + 1, "the candidates"));
    FS_TRY(parent.reserve(tot[0]));
    FS_TRY(dead.reserve(tot[0]));
    FS_TRY(count.reserve(tot[0]));
    FS_TRY(keep.reserve(tot[0]));
    FS_TRY(pos.reserve(tot[0]));
    FS_HIP(hipMemsetAsync(count.p, 0, tot[0] * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(keep.p, 0, tot[0] * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_bun_cands, dim3(blocks_of(tot[0], kRunBlock)), blk, 0, s, f[k],
                       cand_off.p, (uint64_t)tot[0], prune, parent.p, dead.p);
    FS_TRY(clk.mark(m0 + 1, s));
    hipLaunchKernelGGL(k_bun_count, dim3((uint32_t)tot[1]), dim3(kBlock), 0, s, a, f[k],
                       cand_off.p, item_off.p, dead.p, count.p, keep.p);
    FS_TRY(clk.mark(m0 + 2, s));
    hipLaunchKernelGGL(k_pairs_scan<uint32_t>, dim3(1), dim3(kScanBlock), 0, s, keep.p,
                       (uint64_t)tot[0], pos.p, reinterpret_cast<uint32_t*>(totals.p));
    FS_HIP(hipGetLastError());
    uint32_t kept = 0;
    FS_HIP(hipMemcpyAsync(&kept, totals.p, sizeof kept, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    levels[k - 1].frequent = kept;
    t[0] = clk.elapsed(m0, m0 + 1);
    t[1] = clk.elapsed(m0 + 1, m0 + 2);
    if (!kept) return FS_OK;
    FS_TRY(room((uint64_t)kept * (k + 1 + 4) * 4, 0, k + 1, "the list"));
    FS_TRY(lv[k + 1].reserve(kept, k + 1));
    f[k + 1] = lv[k + 1].view(kept, k + 1);
    hipLaunchKernelGGL(k_bun_place, dim3(blocks_of(tot[0], kRunBlock)), blk, 0, s, f[k],
                       f[k + 1], cand_off.p, (uint64_t)tot[0], parent.p, count.p, keep.p, pos.p);
    if (k + 1 <= max_size)
      hipLaunchKernelGGL(k_bun_first, dim3(blocks_of(kept, kRunBlock)), blk, 0, s, a, f[k + 1]);
    FS_TRY(clk.mark(m0 + 3, s));
    hipLaunchKernelGGL(k_bun_mark, dim3(blocks_of((uint64_t)kept * (k + 1), kRunBlock)), blk, 0,
                       s, f[k], f[k + 1]);
    FS_TRY(clk.mark(m0 + 4, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t[2] = clk.elapsed(m0 + 2, m0 + 3);
    t[3] = clk.elapsed(m0 + 3, m0 + 4);
    return FS_OK;
  }

  // the n_sets records into d_sets (finished on return)
  int write(fs_bundle* d_sets, hipStream_t s) {
    uint64_t base = 0;
    FS_TRY(clk.mark(45, s));
    for (uint32_t k = 2; k <= max_size; ++k) {
      if (!f[k].n) continue;
      hipLaunchKernelGGL(k_bun_emit, dim3(blocks_of(f[k].n, kRunBlock)), dim3(kRunBlock), 0, s,
                         f[k], (const uint32_t*)a.r.work_of, a.r.n_active, d_sets, base);
      base += f[k].n;
    }
    FS_TRY(clk.mark(46, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[kTimes - 2] += clk.elapsed(45, 46);
    return FS_OK;
  }

  void sum_times() {
    double all = 0.0;
    for (int k = 0; k + 1 < kTimes; ++k) all += t_ms[k];
    t_ms[kTimes - 1] = all;
  }
};

// the rules both entry points share
int bun_check(uint64_t n_rows, uint32_t n_script, const void* unit_of, uint32_t n_units,
              uint32_t min_words, uint32_t min_all, uint32_t max_size, const void* units,
              const void* levels, const void* sets, uint64_t cap, uint64_t* n_sets) {
  if (!n_sets || !levels || (n_units && !units) || (cap && !sets) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_all == 0) {
    fs_set_error("min_words and min_all must be at least 1");
    return FS_E_INVALID;
  }
  if (max_size < 2 || max_size > FS_BUNDLES_MAX_SIZE) {
    fs_set_error("max_size %u: 2 to %u", max_size, FS_BUNDLES_MAX_SIZE);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("bundles", n_rows, n_script));
  *n_sets = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_bundles(int device, const uint32_t* work, const uint32_t* fan_ix,
                          const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                          uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                          uint32_t min_words, uint32_t max_gap, uint32_t min_all,
                          uint32_t max_size, fs_bundle_unit* units, fs_bundle_level* levels,
                          fs_bundle* sets, uint64_t cap, uint64_t* n_sets) {
  FS_TRY(bun_check(n_rows, n_script, unit_of, n_units, min_words, min_all, max_size, units,
                   levels, sets, cap, n_sets));
  BunJob job;
  if (!n_rows || !n_units) {
    job.max_size = max_size;
    job.blank_levels();
    for (double& t : t_ms) t = 0.0;
    const fs_bundle_unit none{0u, 0u, 0u, 0u};
    for (uint32_t u = 0; u < n_units; ++u) units[u] = none;
    for (uint32_t k = 0; k < max_size; ++k) levels[k] = job.levels[k];
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_unit_of;
  DBuf<fs_bundle_unit> d_units;
  DBuf<fs_bundle> d_sets;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n_script, nullptr));
  FS_TRY(d_units.reserve(n_units));
  FS_TRY(job.mine(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap,
                  min_all, max_size, d_units.p, nullptr));
  FS_TRY(copy_out(units, d_units, n_units));
  for (uint32_t k = 0; k < max_size; ++k) levels[k] = job.levels[k];
  *n_sets = job.n_sets;
  job.sum_times();
  if (job.n_sets > cap) return FS_E_CAPACITY;
  if (job.n_sets) {
    FS_TRY(d_sets.reserve(job.n_sets));
    FS_TRY(job.write(d_sets.p, nullptr));
    FS_TRY(copy_out(sets, d_sets, job.n_sets));
    job.sum_times();
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_bundles_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                               uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                               uint32_t min_words, uint32_t max_gap, uint32_t min_all,
                               uint32_t max_size, fs_bundle_unit* d_units,
                               fs_bundle_level* d_levels, fs_bundle* d_sets, uint64_t cap,
                               uint64_t* n_sets) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: bundles take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(bun_check(n_rows, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, min_all,
                   max_size, d_units, d_levels, d_sets, cap, n_sets));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 15) || ((uintptr_t)d_levels & 7) || ((uintptr_t)d_sets & 15)) {
    fs_set_error("d_rows, d_units and d_sets must be 16-byte aligned device pointers, "
                 "d_levels 8-byte and d_unit_of 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  BunJob job;
  FS_TRY(job.mine(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                  min_words, max_gap, min_all, max_size, d_units, ix->stream));
  FS_HIP(hipMemcpyAsync(d_levels, job.levels, max_size * sizeof(fs_bundle_level),
                        hipMemcpyHostToDevice, ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  *n_sets = job.n_sets;
  job.sum_times();
  if (job.n_sets > cap) return FS_E_CAPACITY;
  if (job.n_sets) FS_TRY(job.write(d_sets, ix->stream));
  job.sum_times();
  return FS_OK;
}

extern "C" int fs_bundles_times(double* ms) {
  return times_out(ms, t_ms, kTimes);
}
