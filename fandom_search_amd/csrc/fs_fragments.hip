// fs_fragments.hip -- `ao3.py fragments`: the phrases the fan works quote word for word, the
// closed frequent intervals of the script (fs_fragments, fs_fragments_rows in
// include/fandom_search.h).  S(a, b) is the number of active works whose coverage holds every
// word of [a, b]; [a, b] is listed when its length is inside [min_length, max_words], S >=
// min_works, and a word more on either side loses a work.
//
// A run is a maximal stretch of consecutive words in one work's coverage.  Row r of a table is
// the length d + 1 with d = d0 + r, d0 = min_length - 1; START[r][a] counts the runs that start
// at a and reach a + d, END[r][a] those that end at a + d and start at or before a.  Then
//   S(a, a + d) = sum of START[r][a'] over a' <= a  -  sum of END[r][a'] over a' < a
// and [a, a + d] is closed exactly when START[r][a] > 0 and END[r][a] > 0: a run
// [f, l] touches START[r][f] and END[r][l - d] for d < min(l - f + 1, max_words) and nothing else.
//
// Every output is an integer, sums and minima in any order.  Separate launches; no workgroup
// waits on another:
//   CoverJob::number / reserve / cover   the passages, the active works, the coverage
//   k_frag_runs      a wave per tile of 64 works and chunk of coverage words, a lane per work: the
//                    0 -> 1 transitions with the carry of the word in front, each run followed to
//                    its end and appended to the list (one counter add per wave and word); per
//                    work its runs and its longest one
//   k_frag_dedup     a lane per run: the distinct (first, last) with their runs and their smallest
//                    work, a hash table settled by comparing keys, equal keys of a wave entered
//                    as one (FS_FRAGMENTS_DEDUP=0: skipped)
//   k_frag_spread    a lane finds a distinct run (or, without the dedupe, a run), the wave takes
//                    them in turn with its lanes over d: START, END, the first work, the exact runs
//   k_frag_rows<0>   a workgroup per row: both sums along a in one scan of 64-bit pairs, the
//                    listed cells counted per (row, chunk of 1024 words)
//   k_pairs_scan     their offsets: the fragments come out in (words, first) order
//   k_frag_rows<1>   the same scan again: the fragments written; START becomes the number of
//                    listed cells up to and including a, END becomes S
//   k_frag_held      a wave per run, lanes over d: the listed cells inside it from two reads of
//                    the prefix counts per row; whether the run itself is listed
//   k_frag_works     a lane per active work: its fs_fragment_work
//
// The tables are row-major, [row][script word]: the scans read them coalesced, the spread
// writes a column of them per run.
#include "fs_tiles.h"

namespace {

constexpr uint32_t kRunsChunk = 16;                   // coverage words a wave of k_frag_runs takes
constexpr unsigned long long kNoKey = ~0ull;

struct FragArgs : CoverArgs {
  uint32_t d0, n_rows_t;        // first d, rows of a table
  uint32_t min_works, min_length, max_words;
  uint32_t k_chunks;            // chunks of kRunsChunk coverage words
  uint32_t a_chunks;            // chunks of kScanBlock script words
  uint32_t list_cap, slots, hash_mask;
  uint32_t* n_list;             // runs appended so far
  uint32_t* list_w;             // [list_cap] active number, first, last of a run
  uint32_t* list_f;
  uint32_t* list_l;
  unsigned long long* keys;     // [slots] first << 32 | last, kNoKey: empty
  uint32_t* key_cnt;            // [slots] runs with the key
  uint32_t* key_min;            // [slots] smallest active number among them
  uint32_t* start;              // [n_rows_t][n_script]; after k_frag_rows<1>: listed cells <= a
  uint32_t* end;                // the same; after k_frag_rows<1>: S
  uint32_t* first;              // smallest active number with a run from a that reaches a + d
  uint32_t* exact;              // runs that are exactly [a, a + d]
  uint32_t* cnt;                // [n_rows_t][a_chunks] listed cells
  unsigned long long* off;      // the same, scanned
  unsigned long long* total;
  uint32_t* wruns;              // [n_tiles * 64] per active work
  uint32_t* wheld;
  uint32_t* wexact;
  unsigned long long* wtop;     // length << 32 | ~first of the longest run
  fs_fragment* frags;
  fs_fragment_work* works;
};

__device__ inline uint32_t frag_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

// blockIdx.x * 4 + wave = tile * k_chunks + chunk; lane r is active work tile * 64 + r (rows
// past the last active work are zero: no runs)
__global__ __launch_bounds__(kRunBlock) void k_frag_runs(FragArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t gw = (uint64_t)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  const uint32_t t = (uint32_t)(gw / a.k_chunks), c = (uint32_t)(gw % a.k_chunks);
  if (t >= a.n_tiles) return;                              // (wave-uniform)
  const size_t ai = (size_t)t * kTile + lane;
  const unsigned long long* row = a.cov + (size_t)t * a.nk * kTile + lane;
  const uint32_t k0 = c * kRunsChunk;
  const uint32_t k1 = a.nk - k0 < kRunsChunk ? a.nk : k0 + kRunsChunk;
  unsigned long long carry = k0 ? row[(size_t)(k0 - 1) * kTile] >> 63 : 0ull;
  uint32_t mine = 0;
  unsigned long long top = 0;
  for (uint32_t k = k0; k < k1; ++k) {
    const unsigned long long x = row[(size_t)k * kTile];
    unsigned long long starts = x & ~((x << 1) | carry);
    carry = x >> 63;
    const uint32_t here = (uint32_t)__popcll(starts);
    const uint32_t upto = wave_scan(here);
    const uint32_t all = lane_u32(upto, 63);
    if (!all) continue;                                    // (wave-uniform)
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(a.n_list, all);
    at = lane_u32(at, 0) + upto - here;
    while (starts) {
      const uint32_t s = (uint32_t)__builtin_ctzll(starts);
      starts &= starts - 1;
      // the first word behind s that the work does not cover
      const unsigned long long z = s == 63 ? 0ull : ~x & (~0ull << (s + 1));
      uint32_t last;
      if (z) {
        last = (k << 6) + (uint32_t)__builtin_ctzll(z) - 1;
      } else {
        uint32_t kk = k + 1;
        for (;;) {
          if (kk >= a.nk) {
            last = a.n_script - 1;
            break;
          }
          const unsigned long long y = ~row[(size_t)kk * kTile];
          if (y) {
            last = (kk << 6) + (uint32_t)__builtin_ctzll(y) - 1;
            break;
          }
          ++kk;
        }
      }
      const uint32_t f = (k << 6) + s;
      if (last >= a.n_script) last = a.n_script - 1;       // (never: no bit behind the script)
      if (at < a.list_cap) {                               // (always: a run starts a passage)
        a.list_w[at] = (uint32_t)ai;
        a.list_f[at] = f;
        a.list_l[at] = last;
      }
      ++at;
      ++mine;
      const unsigned long long key = ((unsigned long long)(last - f + 1) << 32) | (uint32_t)~f;
      if (key > top) top = key;
    }
  }
  if (mine) {
    atomicAdd(&a.wruns[ai], mine);
    atomicMax(&a.wtop[ai], top);
  }
}

// one lane per run of the list.  The lanes of a wave that hold the same (first, last) go to
// the table as one: neighbours in the list are the 64 works of a tile at one coverage word, and
// on a famous line they all hold the same run.
__global__ __launch_bounds__(kRunBlock) void k_frag_dedup(FragArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_list = *a.n_list < a.list_cap ? *a.n_list : a.list_cap;
  const bool have = r < n_list;
  unsigned long long key = kNoKey;
  uint32_t w = FS_NONE, mine = 0;                          // mine: the runs this lane enters
  if (have) {
    key = ((unsigned long long)a.list_f[r] << 32) | a.list_l[r];
    w = a.list_w[r];
  }
  uint64_t todo = __ballot(have);
  while (todo) {                                           // (wave-uniform)
    const int from = __builtin_ctzll(todo);
    const unsigned long long k = __shfl(key, from);
    const bool same = have && key == k;
    const uint64_t group = __ballot(same);
    todo &= ~group;
    uint32_t least = same ? w : FS_NONE;
    for (uint32_t d = 32; d; d >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)least, (int)d);
      if (o < least) least = o;
    }
    if (lane == (uint32_t)from) {                          // the group's first lane enters it
      mine = (uint32_t)__popcll(group);
      w = least;
    }
  }
  if (!mine) return;
  uint32_t s = (frag_hash(key) & a.hash_mask) & (a.slots - 1);
  for (;;) {                                               // (slots >= 2 * list_cap: ends)
    const unsigned long long was = atomicCAS(&a.keys[s], kNoKey, key);
    if (was == kNoKey || was == key) break;
    s = (s + 1) & (a.slots - 1);
  }
  atomicAdd(&a.key_cnt[s], mine);
  atomicMin(&a.key_min[s], w);
}

// kDedup: a lane per slot of the table; else a lane per run of the list.  The wave then takes
// what its lanes found one at a time, lanes over d.
template <int kDedup>
__global__ __launch_bounds__(kRunBlock) void k_frag_spread(FragArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  bool have = false;
  uint32_t f = 0, l = 0, cnt = 0, mw = 0;
  if (kDedup) {
    if (i < a.slots) {
      const unsigned long long key = a.keys[i];
      if (key != kNoKey) {
        have = true;
        f = (uint32_t)(key >> 32);
        l = (uint32_t)key;
        cnt = a.key_cnt[i];
        mw = a.key_min[i];
      }
    }
  } else {
    const uint32_t n_list = *a.n_list < a.list_cap ? *a.n_list : a.list_cap;
    if (i < n_list) {
      have = true;
      f = a.list_f[i];
      l = a.list_l[i];
      cnt = 1;
      mw = a.list_w[i];
    }
  }
  uint64_t todo = __ballot(have);
  const uint32_t d1 = a.d0 + a.n_rows_t - 1;
  while (todo) {
    const int from = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t bf = (uint32_t)__shfl((int)f, from), bl = (uint32_t)__shfl((int)l, from);
    const uint32_t bc = (uint32_t)__shfl((int)cnt, from), bw = (uint32_t)__shfl((int)mw, from);
    if (bl < bf || bl >= a.n_script) continue;             // (never)
    const uint32_t dl = bl - bf;                           // d of the run itself
    const uint32_t dm = dl < d1 ? dl : d1;
    for (uint64_t d = (uint64_t)a.d0 + lane; d <= dm; d += 64) {
      const size_t at = (size_t)(d - a.d0) * a.n_script;
      atomicAdd(&a.start[at + bf], bc);
      atomicMin(&a.first[at + bf], bw);
      atomicAdd(&a.end[at + bl - (uint32_t)d], bc);
    }
    if (lane == 0 && dl >= a.d0 && dl <= d1)
      atomicAdd(&a.exact[(size_t)(dl - a.d0) * a.n_script + bf], bc);
  }
}

// blockIdx.x = row.  The row in chunks of kScanBlock words in turn: one scan of (START, END) as
// a 64-bit pair gives both sums (each below 2^32: no more runs than records), one rank the
// places of the listed cells.  kPlace 0: the counts; 1: the fragments, START := listed cells up
// to and including a, END := S.
template <int kPlace>
__global__ __launch_bounds__(kScanBlock) void k_frag_rows(FragArgs a) {
  __shared__ unsigned long long s_w[kScanBlock / 64];
  __shared__ uint32_t s_r[kScanBlock / 64];
  const uint32_t row = blockIdx.x, d = a.d0 + row;
  const size_t base = (size_t)row * a.n_script;
  unsigned long long carry = 0;
  uint32_t listed_before = 0;
  for (uint32_t c = 0; c < a.a_chunks; ++c) {
    const uint32_t j = c * kScanBlock + threadIdx.x;
    uint32_t st = 0, en = 0;
    if (j < a.n_script) {
      st = a.start[base + j];
      en = a.end[base + j];
    }
    unsigned long long sum;
    const unsigned long long pre =
        carry + block_scan_open<kScanBlock>(((unsigned long long)st << 32) | en, s_w, &sum);
    const uint32_t S = (uint32_t)(pre >> 32) + st - (uint32_t)pre;
    const bool listed = st && en && S >= a.min_works;
    uint32_t rank, total;
    block_rank<kScanBlock>(listed, s_r, &rank, &total);
    if (kPlace) {
      if (listed) {
        const unsigned long long pos = a.off[(size_t)row * a.a_chunks + c] + rank;
        uint4* p = reinterpret_cast<uint4*>(a.frags + pos);
        p[0] = make_uint4(j, j + d, S, a.exact[base + j]);
        p[1] = make_uint4(st, en, a.work_of[a.first[base + j]], 0u);
      }
      if (j < a.n_script) {
        a.start[base + j] = listed_before + rank + (listed ? 1u : 0u);
        a.end[base + j] = S;
      }
    } else if (threadIdx.x == 0) {
      a.cnt[(size_t)row * a.a_chunks + c] = total;
    }
    carry += sum;
    listed_before += total;
  }
}

// a lane per run of the list; the wave takes them in turn, lanes over d (after k_frag_rows<1>)
__global__ __launch_bounds__(kRunBlock) void k_frag_held(FragArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n_list = *a.n_list < a.list_cap ? *a.n_list : a.list_cap;
  uint32_t f = 0, l = 0, w = 0;
  if (i < n_list) {
    f = a.list_f[i];
    l = a.list_l[i];
    w = a.list_w[i];
  }
  uint64_t todo = __ballot(i < n_list);
  const uint32_t d1 = a.d0 + a.n_rows_t - 1;
  while (todo) {
    const int from = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t bf = (uint32_t)__shfl((int)f, from), bl = (uint32_t)__shfl((int)l, from);
    const uint32_t bw = (uint32_t)__shfl((int)w, from);
    if (bl < bf || bl >= a.n_script) continue;             // (never)
    const uint32_t dl = bl - bf, dm = dl < d1 ? dl : d1;
    uint32_t sum = 0;
    for (uint64_t d = (uint64_t)a.d0 + lane; d <= dm; d += 64) {
      const size_t at = (size_t)(d - a.d0) * a.n_script;
      sum += a.start[at + bl - (uint32_t)d] - (bf ? a.start[at + bf - 1] : 0u);
    }
    sum = wave_sum(sum);
    if (lane == 0) {
      if (sum) atomicAdd(&a.wheld[bw], sum);
      if (dl >= a.d0 && dl <= d1) {
        const size_t at = (size_t)(dl - a.d0) * a.n_script;
        if (a.start[at + bf] != (bf ? a.start[at + bf - 1] : 0u)) atomicAdd(&a.wexact[bw], 1u);
      }
    }
  }
}

// one lane per active work (each has a run)
__global__ __launch_bounds__(kRunBlock) void k_frag_works(FragArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.n_active) return;
  const unsigned long long top = a.wtop[w];
  const uint32_t len = (uint32_t)(top >> 32), f = ~(uint32_t)top;
  uint32_t s = FS_NONE;
  if (len >= a.min_length && len <= a.max_words && len - 1 - a.d0 < a.n_rows_t)
    s = a.end[(size_t)(len - 1 - a.d0) * a.n_script + f];
  uint4* p = reinterpret_cast<uint4*>(a.works + w);
  p[0] = make_uint4(a.work_of[w], a.wruns[w], a.covered[w], a.wheld[w]);
  p[1] = make_uint4(a.wexact[w], f, f + len - 1, s);
}

thread_local double t_ms[5];    // runs, spread, list, works, total of the last call

// one call: count() through the numbers of active works and fragments, then write()
struct FragJob {
  CoverJob cj;
  DBuf<uint32_t> n_list, list, tables, cnt, wacc;
  DBuf<unsigned long long> keys, off, total, wtop;
  Clock<8> clk;
  FragArgs a{};
  uint64_t n_frags = 0;
  uint32_t dedup = 1;

  // a.n_active and n_frags set (all on `s`, finished on return)
  int count(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
            uint32_t min_words, uint32_t max_gap, uint32_t min_works, uint32_t min_length,
            uint32_t max_words, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.min_works = min_works;
    a.min_length = min_length;
    a.max_words = max_words;
    dedup = env_u32("FS_FRAGMENTS_DEDUP", 1u, 1u);
    const uint32_t bits = env_u32("FS_FRAGMENTS_HASH_BITS", 32u, 32u);
    a.hash_mask = bits >= 32 ? ~0u : (1u << bits) - 1;
    if (!n) return FS_OK;
    FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) return FS_OK;
    // rows d0 .. d1: no interval is longer than the script
    a.d0 = min_length - 1;
    const uint32_t longest = max_words < n_script ? max_words : n_script;
    a.n_rows_t = longest > a.d0 ? longest - a.d0 : 1u;
    a.k_chunks = (a.nk + kRunsChunk - 1) / kRunsChunk;
    a.a_chunks = (n_script + kScanBlock - 1) / kScanBlock;
    a.list_cap = a.n_runs;
    a.slots = 64;
    while (a.slots < 2ull * a.list_cap && a.slots < (1u << 31)) a.slots <<= 1;
    const size_t rows = (size_t)a.n_tiles * kTile;
    const uint64_t cells = (uint64_t)a.n_rows_t * n_script;
    const uint64_t bytes = (uint64_t)rows * a.nk * 8 + (uint64_t)a.list_cap * 12 +
                           (dedup ? (uint64_t)a.slots * 16 : 0) + cells * 16;
    if (bytes > FS_FRAGMENTS_MAX_BYTES || 2ull * a.list_cap > a.slots) {
      fs_set_error("%u lengths (max_words - min_length + 1) x %u script words over %u works "
                   "with a passage: tables of more than %u bytes; lower max_words (--max-words)",
                   a.n_rows_t, n_script, a.n_active, FS_FRAGMENTS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    const uint64_t run_blocks = ((uint64_t)a.n_tiles * a.k_chunks + 3) / 4;
    if (run_blocks > 0x7FFFFFFFull) {
      fs_set_error("%u works with a passage over %u script words: more chunks than a launch "
                   "takes", a.n_active, n_script);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(cj.reserve(a, s));
    FS_TRY(n_list.reserve(1));
    FS_TRY(list.reserve(3 * (size_t)a.list_cap + (dedup ? 2 * (size_t)a.slots : 0)));
    FS_TRY(tables.reserve(4 * (size_t)cells));
    FS_TRY(cnt.reserve((size_t)a.n_rows_t * a.a_chunks));
    FS_TRY(off.reserve((size_t)a.n_rows_t * a.a_chunks));
    FS_TRY(total.reserve(1));
    FS_TRY(wacc.reserve(3 * rows));
    FS_TRY(wtop.reserve(rows));
    FS_HIP(hipMemsetAsync(n_list.p, 0, sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(tables.p, 0, 4 * (size_t)cells * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(tables.p + 2 * (size_t)cells, 0xFF, (size_t)cells * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(wacc.p, 0, 3 * rows * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(wtop.p, 0, rows * sizeof(unsigned long long), s));
    a.n_list = n_list.p;
    a.list_w = list.p;
    a.list_f = list.p + a.list_cap;
    a.list_l = list.p + 2 * (size_t)a.list_cap;
    a.start = tables.p;
    a.end = tables.p + (size_t)cells;
    a.first = tables.p + 2 * (size_t)cells;
    a.exact = tables.p + 3 * (size_t)cells;
    a.cnt = cnt.p;
    a.off = off.p;
    a.total = total.p;
    a.wruns = wacc.p;
    a.wheld = wacc.p + rows;
    a.wexact = wacc.p + 2 * rows;
    a.wtop = wtop.p;
    if (dedup) {
      FS_TRY(keys.reserve(a.slots));
      a.keys = keys.p;
      a.key_cnt = list.p + 3 * (size_t)a.list_cap;         // (behind the run list)
      a.key_min = a.key_cnt + a.slots;
      FS_HIP(hipMemsetAsync(keys.p, 0xFF, (size_t)a.slots * sizeof(unsigned long long), s));
      FS_HIP(hipMemsetAsync(a.key_cnt, 0, (size_t)a.slots * sizeof(uint32_t), s));
      FS_HIP(hipMemsetAsync(a.key_min, 0xFF, (size_t)a.slots * sizeof(uint32_t), s));
    }
    const dim3 blk(kRunBlock);
    const dim3 list_grid(blocks_of(a.list_cap, kRunBlock));
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    hipLaunchKernelGGL(k_frag_runs, dim3((uint32_t)run_blocks), blk, 0, s, a);
    FS_TRY(clk.mark(1, s));
    if (dedup) {
      hipLaunchKernelGGL(k_frag_dedup, list_grid, blk, 0, s, a);
      hipLaunchKernelGGL(k_frag_spread<1>, dim3(blocks_of(a.slots, kRunBlock)), blk, 0, s, a);
    } else {
      hipLaunchKernelGGL(k_frag_spread<0>, list_grid, blk, 0, s, a);
    }
    FS_TRY(clk.mark(2, s));
    hipLaunchKernelGGL(k_frag_rows<0>, dim3(a.n_rows_t), dim3(kScanBlock), 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s, cnt.p,
                       (uint64_t)a.n_rows_t * a.a_chunks, off.p, total.p);
    FS_TRY(clk.mark(3, s));
    FS_HIP(hipGetLastError());
    unsigned long long tot = 0;
    FS_HIP(hipMemcpyAsync(&tot, total.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    n_frags = tot;
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    t_ms[2] = clk.elapsed(2, 3);
    t_ms[4] = t_ms[0] + t_ms[1] + t_ms[2];
    return FS_OK;
  }

  // the n_frags fragments and the a.n_active works (finished on return)
  int write(fs_fragment* d_frags, fs_fragment_work* d_works, hipStream_t s) {
    if (!a.n_active) return FS_OK;
    a.frags = d_frags;
    a.works = d_works;
    const dim3 blk(kRunBlock);
    FS_TRY(clk.mark(4, s));
    hipLaunchKernelGGL(k_frag_rows<1>, dim3(a.n_rows_t), dim3(kScanBlock), 0, s, a);
    FS_TRY(clk.mark(5, s));
    hipLaunchKernelGGL(k_frag_held, dim3(blocks_of(a.list_cap, kRunBlock)), blk, 0, s, a);
    hipLaunchKernelGGL(k_frag_works, dim3(blocks_of(a.n_active, kRunBlock)), blk, 0, s, a);
    FS_TRY(clk.mark(6, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[2] += clk.elapsed(4, 5);
    t_ms[3] = clk.elapsed(5, 6);
    t_ms[4] = t_ms[0] + t_ms[1] + t_ms[2] + t_ms[3];
    return FS_OK;
  }
};

// the rules both entry points share
int fragments_check(uint64_t n_rows, uint32_t n_script, uint32_t min_words, uint32_t min_length,
                    uint32_t max_words, const void* frags, uint64_t frags_cap, uint64_t* n_frags,
                    const void* works, uint64_t works_cap, uint64_t* n_active) {
  if (!n_frags || !n_active || (frags_cap && !frags) || (works_cap && !works)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_length == 0) {
    fs_set_error("min_words and min_length must be at least 1");
    return FS_E_INVALID;
  }
  if (max_words < min_length) {
    fs_set_error("max_words %u below min_length %u", max_words, min_length);
    return FS_E_INVALID;
  }
  if (max_words > FS_FRAGMENTS_MAX_WORDS) {
    fs_set_error("max_words %u: fragments take up to %u", max_words, FS_FRAGMENTS_MAX_WORDS);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(record_limits("fragments", n_rows, n_script));
  *n_frags = 0;
  *n_active = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_fragments(int device, const uint32_t* work, const uint32_t* fan_ix,
                            const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                            uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                            uint32_t min_works, uint32_t min_length, uint32_t max_words,
                            fs_fragment* frags, uint64_t frags_cap, uint64_t* n_frags,
                            fs_fragment_work* works, uint64_t works_cap, uint64_t* n_active) {
  FS_TRY(fragments_check(n_rows, n_script, min_words, min_length, max_words, frags, frags_cap,
                         n_frags, works, works_cap, n_active));
  if (!n_rows) return FS_OK;
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_fragment> d_frags;
  DBuf<fs_fragment_work> d_works;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FragJob job;
  FS_TRY(job.count(rows.p, n, n_works, n_script, min_words, max_gap, min_works, min_length,
                   max_words, nullptr));
  *n_frags = job.n_frags;
  *n_active = job.a.n_active;
  if (job.n_frags > frags_cap || job.a.n_active > works_cap) return FS_E_CAPACITY;
  if (!job.a.n_active) return FS_OK;
  FS_TRY(d_frags.reserve(job.n_frags));
  FS_TRY(d_works.reserve(job.a.n_active));
  FS_TRY(job.write(d_frags.p, d_works.p, nullptr));
  if (job.n_frags) FS_TRY(copy_out(frags, d_frags, job.n_frags));
  FS_TRY(copy_out(works, d_works, job.a.n_active));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_fragments_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                 uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                                 uint32_t min_works, uint32_t min_length, uint32_t max_words,
                                 fs_fragment* d_frags, uint64_t frags_cap, uint64_t* n_frags,
                                 fs_fragment_work* d_works, uint64_t works_cap,
                                 uint64_t* n_active) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: fragments take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(fragments_check(n_rows, (uint32_t)ix->n_script, min_words, min_length, max_words,
                         d_frags, frags_cap, n_frags, d_works, works_cap, n_active));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_frags & 15) ||
      ((uintptr_t)d_works & 15)) {
    fs_set_error("d_rows, d_frags and d_works must be 16-byte aligned device pointers");
    return FS_E_INVALID;
  }
  if (!n_rows) return FS_OK;
  FS_ENTER(ix->device);
  FragJob job;
  FS_TRY(job.count(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                   min_works, min_length, max_words, ix->stream));
  *n_frags = job.n_frags;
  *n_active = job.a.n_active;
  if (job.n_frags > frags_cap || job.a.n_active > works_cap) return FS_E_CAPACITY;
  FS_TRY(job.write(d_frags, d_works, ix->stream));
  return FS_OK;
}

extern "C" int fs_fragments_times(double* ms) {
  return times_out(ms, t_ms, 5);
}
