// fs_matrix.hip -- `ao3.py matrix --engine device`: the n-grams the works x phrases matrix is
// built from (fs_matrix, fs_matrix_rows in include/fandom_search.h).  Records sorted by
// (work, fan_ix); a fan run starts where the work changes or fan_ix is not the previous + 1.
// Inside a fan run only c(v), the number of its records that name script word v, decides the
// spans: a span passes through v only when c(v) == 1, a word named twice
// ends one span and starts the next, every further copy is the span [v, v].  So
//   - v starts a span that goes on when c(v) >= 2 or v - 1 is not named in the run; it ends at
//     the first w > v with c(w) >= 2, or at the last word named without a gap;
//   - v is (c(v) - 2) times the span [v, v] when c(v) >= 2, once more when v - 1 is not named.
// Spans of at least n words count every start a .. b - n + 1 in the counter, pick the first of
// their starts with the largest count, and keep it when no start within n - 1 words in front
// has as large a count and none within n - 1 words behind a larger one.
//
// Separate launches; no workgroup waits on another:
//   k_mx_heads    a lane per record: bounds, order, run heads counted per workgroup, then (after
//                 k_mx_scan) the run of every record and c(run, v) in an open-addressing table
//                 keyed by the pair (equal hashes are settled by comparing keys)
//   k_mx_spans    a lane per table slot: the span that starts there, walked over words with
//                 c == 1, and the single-word spans; spans per run; the counter as a difference
//                 array, two adds a span, summed per workgroup in LDS first where spans share ends
//   k_mx_starts   one workgroup: the counter, the running sum of the differences
//   k_mx_entries  a lane per slot: its spans into their run's stretch of the span list
//   k_mx_pick     a lane per span: its place in the run by (first, last), and, for a span of up
//                 to FS_MATRIX_SMALL starts, its n-gram and the neighbourhood test
//   k_mx_pick_wave  a wave per longer span
//   k_mx_keep     the kept n-grams counted per workgroup, then (after k_mx_scan) placed: the
//                 list is in span order without a sort of the whole
// Every value is an integer and every atomic an integer add, a maximum or a claim whose loser
// reads the winner: no schedule changes a result.
#include "fs_internal.h"
#include "fs_prims.h"
#include "fs_probe.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSmallDefault = 32;
constexpr uint32_t kLongRun = 256;              // runs of this many spans are ranked by a wave
constexpr uint32_t kAgg = 512;                  // LDS entries that gather a workgroup's adds
constexpr uint64_t kNoSlot = ~0ull;

static_assert(sizeof(fs_matrix_ngram) == 8, "fs_matrix");

// status words
enum { kStBad = 0, kStUnsorted = 1, kStRuns = 2, kStSpans = 3, kStLong = 4, kStKept = 5,
       kStWords = 8 };

struct MxArgs {
  uint32_t n, n_works, n_script, ngram;
  uint32_t n_runs, n_spans, small;
  uint64_t slots, mask, hash_mask;  // FS_MATRIX_HASH_BITS: the bits of a key's hash kept
  unsigned long long* tab;       // [slots] run << 32 | script word
  uint32_t* cv;                  // [slots] c(run, v)
  uint32_t* sb;                  // [slots] last word of the kept span that starts here, or FS_NONE
  uint32_t* sm;                  // [slots] kept single-word spans here
  uint32_t* rcnt;                // [workgroups of records] run heads, then their exclusive scan
  uint32_t* rwork;               // [n_runs] the run's work
  uint32_t* rspan;               // [n_runs + 1] kept spans of the run, then their exclusive scan
  uint32_t* rcur;                // [n_runs] spans of the run listed so far
  uint32_t* diff;                // [n_script + 1]
  uint32_t* starts;              // [n_script]
  uint32_t* ea;                  // [n_spans] each, runs in order, a run's spans in any order:
  uint32_t* eb;                  //   first and last word, run, place in span order
  uint32_t* erun;
  uint32_t* epos;
  uint32_t* es;                  // [n_spans] in span order: start of the kept n-gram or FS_NONE
  uint32_t* ew;                  //   and the work
  uint32_t* longs;               // [n_spans] the spans left to k_mx_pick_wave
  uint32_t* kcnt;                // [workgroups of spans] kept n-grams, then their exclusive scan
  uint32_t* status;
  fs_matrix_ngram* out;
};

__device__ inline uint64_t home_of(const MxArgs& a, uint64_t key) {
  return fs_mix64(fs_mix64(key) & a.hash_mask) & a.mask;
}

// the slot of `key` in the finished table, kNoSlot when it has none.  Eight slots are loaded
// at a time (they share a cache line or two) and looked at in probe order.
__device__ inline uint64_t find(const MxArgs& a, uint64_t key) {
  for (uint64_t pos = home_of(a, key);; pos = (pos + 8) & a.mask) {
    unsigned long long cur[8];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) cur[k] = a.tab[(pos + k) & a.mask];
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
      if (cur[k] == key) return (pos + k) & a.mask;
      if (cur[k] == kProbeEmpty) return kNoSlot;
    }
  }
}

// exclusive scan of in[0..nb) into out (which may be in), *total = sum
__global__ __launch_bounds__(kScanBlock) void k_mx_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t nb, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, nb, out, total);
}

// kPlace false: bounds, order and the run heads of this workgroup's 256 records into rcnt;
// true (rcnt holding the scan): the work of every run, c(run, v) counted
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_mx_heads(RowsSrc src, MxArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool head = false, bad = false, unsorted = false;
  uint4 s = make_uint4(0, 0, 0, 0);
  if (i < a.n) {
    s = src.key(i);
    head = true;
    bad = s.x >= a.n_works || s.z >= a.n_script;
    if (i > 0) {
      const uint4 r = src.key(i - 1);
      unsorted = s.x < r.x || (s.x == r.x && s.y < r.y);
      head = s.x != r.x || (uint64_t)s.y != (uint64_t)r.y + 1;    // no 32-bit wrap
    }
  }
  uint32_t rank, total;
  block_rank<kBlock>(head, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.rcnt[blockIdx.x] = total;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStBad], 1u);
    if (__ballot(unsorted) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStUnsorted], 1u);
  } else if (i < a.n) {
    const uint32_t run = a.rcnt[blockIdx.x] + rank - (head ? 0u : 1u);   // record 0 is a head
    if (head) a.rwork[run] = s.x;
    const unsigned long long key = (unsigned long long)run << 32 | s.z;
    bool inserted;
    const uint64_t slot = fs_probe_insert(
        a.tab, a.mask, home_of(a, key), key,
        [key](unsigned long long cur) { return cur == key; }, &inserted);
    atomicAdd(&a.cv[slot], 1u);
  }
}

// delta onto diff[at]: gathered in the workgroup's LDS entry of `at` when it has or can claim
// one, else added at once
__device__ inline void agg_add(uint32_t* s_key, uint32_t* s_val, uint32_t* diff, uint32_t at,
                               uint32_t delta) {
  const uint32_t h = (at * 2654435761u) >> 23;             // 9 bits: kAgg entries
  const uint32_t k = atomicCAS(&s_key[h], FS_NONE, at);
  if (k == FS_NONE || k == at) atomicAdd(&s_val[h], delta);
  else atomicAdd(&diff[at], delta);
}

__global__ __launch_bounds__(kBlock) void k_mx_spans(MxArgs a) {
  __shared__ uint32_t s_key[kAgg], s_val[kAgg];
  static_assert(kAgg == 512, "agg_add keeps 9 bits");
  for (uint32_t h = threadIdx.x; h < kAgg; h += kBlock) {
    s_key[h] = FS_NONE;
    s_val[h] = 0;
  }
  __syncthreads();
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const unsigned long long key = slot < a.slots ? a.tab[slot] : kProbeEmpty;
  if (key != kProbeEmpty) {
    const uint32_t run = (uint32_t)(key >> 32), v = (uint32_t)key, c = a.cv[slot];
    const bool prev = v > 0 && find(a, key - 1) != kNoSlot;
    uint32_t m = c >= 2 ? c - 2 + (prev ? 0u : 1u) : 0u;
    uint32_t b = FS_NONE;
    if (c >= 2 || !prev) {
      b = v;
      while (b + 1 < a.n_script) {
        const uint64_t t = find(a, (unsigned long long)run << 32 | (b + 1));
        if (t == kNoSlot) break;
        ++b;
        if (a.cv[t] >= 2) break;
      }
      if ((uint64_t)(b - v) + 1 < a.ngram) b = FS_NONE;
    }
    if (a.ngram != 1) m = 0;
    a.sb[slot] = b;
    a.sm[slot] = m;
    const uint32_t spans = m + (b != FS_NONE ? 1u : 0u);
    if (spans) atomicAdd(&a.rspan[run], spans);
    if (b != FS_NONE) {                          // starts v .. b - n + 1
      agg_add(s_key, s_val, a.diff, v, 1u);
      agg_add(s_key, s_val, a.diff, b - a.ngram + 2, 0u - 1u);
    }
    if (m) {
      agg_add(s_key, s_val, a.diff, v, m);
      agg_add(s_key, s_val, a.diff, v + 1, 0u - m);
    }
  } else if (slot < a.slots) {
    a.sb[slot] = FS_NONE;
    a.sm[slot] = 0;
  }
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < kAgg; h += kBlock)
    if (s_key[h] != FS_NONE && s_val[h]) atomicAdd(&a.diff[s_key[h]], s_val[h]);
}

// starts[s] = diff[0] + .. + diff[s] (sums wrap back: a count is at most the number of spans)
__global__ __launch_bounds__(kScanBlock) void k_mx_starts(MxArgs a) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  const uint32_t* diff = a.diff;
  uint32_t* starts = a.starts;
  scan_chunks<1, uint32_t, uint32_t>(
      a.n_script, [diff](uint64_t j) { return diff[j]; },
      [starts](uint64_t j, uint32_t pre, uint32_t x) { starts[j] = pre + x; }, s_w);
}

__global__ __launch_bounds__(kBlock) void k_mx_entries(MxArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot >= a.slots) return;
  const uint32_t b = a.sb[slot], m = a.sm[slot];
  const uint32_t spans = m + (b != FS_NONE ? 1u : 0u);
  if (!spans) return;
  const unsigned long long key = a.tab[slot];
  const uint32_t run = (uint32_t)(key >> 32), v = (uint32_t)key;
  uint32_t e = a.rspan[run] + atomicAdd(&a.rcur[run], spans);
  for (uint32_t k = 0; k < m; ++k, ++e) {
    a.ea[e] = v;
    a.eb[e] = v;
    a.erun[e] = run;
  }
  if (b != FS_NONE) {
    a.ea[e] = v;
    a.eb[e] = b;
    a.erun[e] = run;
  }
}

__device__ inline uint64_t span_key(uint32_t first, uint32_t last) {
  return (uint64_t)first << 32 | last;
}

// the n-gram of the span [a0, b0] by one lane: FS_NONE when the neighbourhood drops it
__device__ inline uint32_t pick_lane(const MxArgs& a, uint32_t a0, uint32_t b0) {
  uint32_t best = 0, s = a0;
  for (uint32_t t = a0; t <= b0 + 1 - a.ngram; ++t) {
    const uint32_t c = a.starts[t];
    if (c > best) {                              // the first maximum
      best = c;
      s = t;
    }
  }
  const uint32_t reach = a.ngram - 1;
  const uint32_t lo = s >= reach ? s - reach : 0u;
  const uint64_t top = (uint64_t)s + reach;
  const uint32_t hi = top < a.n_script ? (uint32_t)top : a.n_script - 1;
  bool ok = true;
  for (uint32_t t = lo; t < s; ++t) ok &= a.starts[t] < best;
  for (uint32_t t = s + 1; t <= hi; ++t) ok &= a.starts[t] <= best;
  return ok ? s : FS_NONE;
}

// the same by a wave (a0, b0 wave-uniform): a start is compared as (count, ~start), so that a
// plain maximum is the first of the largest
__device__ inline uint32_t pick_wave(const MxArgs& a, uint32_t a0, uint32_t b0, uint32_t lane) {
  uint64_t k = 0;
  const uint32_t last = b0 + 1 - a.ngram;
  for (uint64_t t = (uint64_t)a0 + lane; t <= last; t += 64) {
    const uint64_t cand = (uint64_t)a.starts[t] << 32 | (uint32_t)~(uint32_t)t;
    if (cand > k) k = cand;
  }
  k = wave_max(k);
  const uint32_t best = (uint32_t)(k >> 32), s = ~(uint32_t)k;
  const uint32_t reach = a.ngram - 1;
  const uint32_t lo = s >= reach ? s - reach : 0u;
  const uint64_t top = (uint64_t)s + reach;
  const uint32_t hi = top < a.n_script ? (uint32_t)top : a.n_script - 1;
  bool bad = false;
  for (uint64_t t = (uint64_t)lo + lane; t <= hi; t += 64) {
    const uint32_t c = a.starts[t];
    bad |= t < s ? c >= best : c > best;
  }
  return __ballot(bad) ? FS_NONE : s;
}

// a lane per span of the list: its place among its run's spans by (first, last) -- equal spans
// give equal n-grams, the list order settles them -- and the short spans' n-grams
__global__ __launch_bounds__(kBlock) void k_mx_pick(MxArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = e < a.n_spans;
  uint32_t a0 = 0, b0 = 0, run = 0, first = 0, len = 0, rank = 0;
  if (live) {
    a0 = a.ea[e];
    b0 = a.eb[e];
    run = a.erun[e];
    first = a.rspan[run];
    len = a.rspan[run + 1] - first;
  }
  const uint64_t mine = span_key(a0, b0);
  const bool is_long = live && len >= kLongRun;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = lane_u32(first, j), lj = lane_u32(len, j);
    const uint32_t ej = lane_u32((uint32_t)e, j);
    const uint64_t kj = span_key(lane_u32(a0, j), lane_u32(b0, j));
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) {
      const uint64_t other = span_key(a.ea[fj + k], a.eb[fj + k]);
      before += other < kj || (other == kj && fj + k < ej) ? 1u : 0u;
    }
    before = wave_sum(before);
    if ((int)lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k) {
      const uint64_t other = span_key(a.ea[first + k], a.eb[first + k]);
      rank += other < mine || (other == mine && first + k < e) ? 1u : 0u;
    }
  if (!live) return;
  const uint32_t pos = first + rank;
  a.epos[e] = pos;
  a.ew[pos] = a.rwork[run];
  if (b0 - a0 + 2 - a.ngram <= a.small) a.es[pos] = pick_lane(a, a0, b0);
  else a.longs[atomicAdd(&a.status[kStLong], 1u)] = (uint32_t)e;
}

__global__ __launch_bounds__(64) void k_mx_pick_wave(MxArgs a) {
  const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.longs[blockIdx.x]);
  const uint32_t a0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.ea[e]);
  const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.eb[e]);
  const uint32_t s = pick_wave(a, a0, b0, threadIdx.x);
  if (threadIdx.x == 0) a.es[a.epos[e]] = s;
}

// kPlace false: the kept n-grams of this workgroup's 256 spans into kcnt; true: to their places
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_mx_keep(MxArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t s = p < a.n_spans ? a.es[p] : FS_NONE;
  uint32_t rank, total;
  block_rank<kBlock>(s != FS_NONE, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.kcnt[blockIdx.x] = total;
  } else if (s != FS_NONE) {
    a.out[a.kcnt[blockIdx.x] + rank] = fs_matrix_ngram{a.ew[p], s};
  }
}

// runs (checks, heads, the table), spans (ends, difference array), counter, pick (list, places,
// n-grams), place, total of the last call
thread_local double t_ms[6];

uint64_t mx_hash_mask() {
  const char* e = getenv("FS_MATRIX_HASH_BITS");   // diagnostic: k bits of a hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  if (k <= 0) return 0ull;
  return k >= 64 ? ~0ull : (1ull << k) - 1;
}

// the rules both entry points share; *done when nothing is left to do
int mx_check(uint64_t n_rows, uint32_t n_script, uint32_t ngram, const void* out, uint64_t cap,
             uint64_t* n_spans, uint64_t* n_kept, bool* done) {
  *done = false;
  if (!n_spans || !n_kept || (cap && !out)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ngram == 0) {
    fs_set_error("ngram must be at least 1");
    return FS_E_INVALID;
  }
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: matrix takes fewer than 2^32", (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  if (n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("n_script %u: matrix takes up to %u", n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  const uint64_t bytes = fs_probe_slots(n_rows) * 20 + n_rows * 40 + ((uint64_t)n_script + 1) * 8;
  if (n_rows && bytes > FS_MATRIX_MAX_BYTES) {
    fs_set_error("%llu records need tables of %llu bytes: matrix takes up to %u",
                 (unsigned long long)n_rows, (unsigned long long)bytes, FS_MATRIX_MAX_BYTES);
    return FS_E_UNSUPPORTED;
  }
  *n_spans = 0;
  *n_kept = 0;
  *done = n_rows == 0;
  return FS_OK;
}

struct MxScratch {
  DBuf<uint32_t> status, slot_words, rcnt, run_words, diff, starts, span_words, kcnt;
  DBuf<unsigned long long> tab;
};

// d_starts (when not null) and d_out written, *n_spans and *n_kept set; d_out untouched on
// FS_E_CAPACITY (all on `s`, finished on return)
int mx_run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script, uint32_t ngram,
           uint32_t* d_starts, fs_matrix_ngram* d_out, uint64_t cap, uint64_t* n_spans,
           uint64_t* n_kept, hipStream_t s) {
  const RowsSrc src{d_rows};
  for (double& t : t_ms) t = 0.0;
  if (!n_works || !n_script) {
    fs_set_error("a work >= n_works or a script index >= n_script");
    return FS_E_INVALID;
  }
  MxScratch k;
  MxArgs a{};
  Clock<6> clk;
  a.n = n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.ngram = ngram;
  // FS_MATRIX_SMALL: a diagnostic, read on each call (0: every span goes to a wave)
  a.small = env_u32("FS_MATRIX_SMALL", kSmallDefault, 0xFFFFFFFFu);
  a.hash_mask = mx_hash_mask();
  a.slots = fs_probe_slots(n);
  a.mask = a.slots - 1;
  a.out = d_out;
  const dim3 blk(kBlock);
  const uint32_t rec_blocks = blocks_of(n, kBlock), slot_blocks = blocks_of(a.slots, kBlock);
  FS_TRY(k.status.reserve(kStWords));
  FS_TRY(k.rcnt.reserve(rec_blocks));
  a.status = k.status.p;
  a.rcnt = k.rcnt.p;
  FS_HIP(hipMemsetAsync(a.status, 0, kStWords * sizeof(uint32_t), s));
  FS_TRY(clk.mark(0, s));
  hipLaunchKernelGGL((k_mx_heads<false>), dim3(rec_blocks), blk, 0, s, src, a);
  hipLaunchKernelGGL(k_mx_scan, dim3(1), dim3(kScanBlock), 0, s, a.rcnt, a.rcnt, rec_blocks,
                     a.status + kStRuns);
  FS_HIP(hipGetLastError());
  uint32_t st[kStWords];
  FS_HIP(hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[kStBad]) {
    fs_set_error("a work >= n_works or a script index >= n_script");
    return FS_E_INVALID;
  }
  if (st[kStUnsorted]) {
    fs_set_error("records are not sorted by (work, fan_ix)");
    return FS_E_INVALID;
  }
  a.n_runs = st[kStRuns];
  const size_t nr = a.n_runs;

  // c(run, v)
  FS_TRY(k.tab.reserve(a.slots));
  FS_TRY(k.slot_words.reserve(3 * a.slots));
  FS_TRY(k.run_words.reserve(3 * nr + 1));
  FS_TRY(k.diff.reserve((size_t)n_script + 1));
  a.tab = k.tab.p;
  a.cv = k.slot_words.p;
  a.sb = k.slot_words.p + a.slots;
  a.sm = k.slot_words.p + 2 * a.slots;
  a.rwork = k.run_words.p;
  a.rcur = k.run_words.p + nr;
  a.rspan = k.run_words.p + 2 * nr;
  a.diff = k.diff.p;
  if (d_starts) {
    a.starts = d_starts;
  } else {
    FS_TRY(k.starts.reserve(n_script));
    a.starts = k.starts.p;
  }
  FS_HIP(hipMemsetAsync(a.tab, 0xFF, a.slots * sizeof(unsigned long long), s));
  FS_HIP(hipMemsetAsync(a.cv, 0, a.slots * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(a.rcur, 0, (2 * nr + 1) * sizeof(uint32_t), s));       // and rspan
  FS_HIP(hipMemsetAsync(a.diff, 0, ((size_t)n_script + 1) * sizeof(uint32_t), s));
  hipLaunchKernelGGL((k_mx_heads<true>), dim3(rec_blocks), blk, 0, s, src, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(1, s));

  // the spans, their number per run, the counter
  hipLaunchKernelGGL(k_mx_spans, dim3(slot_blocks), blk, 0, s, a);
  hipLaunchKernelGGL(k_mx_scan, dim3(1), dim3(kScanBlock), 0, s, a.rspan, a.rspan,
                     a.n_runs + 1, a.status + kStSpans);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(2, s));
  hipLaunchKernelGGL(k_mx_starts, dim3(1), dim3(kScanBlock), 0, s, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(3, s));
  FS_HIP(hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  a.n_spans = st[kStSpans];
  *n_spans = a.n_spans;
  const size_t ns = a.n_spans;
  bool fits = true;
  if (ns) {
    // the n-grams
    const uint32_t span_blocks = blocks_of(ns, kBlock);
    FS_TRY(k.span_words.reserve(7 * ns));
    FS_TRY(k.kcnt.reserve(span_blocks));
    a.ea = k.span_words.p;
    a.eb = k.span_words.p + ns;
    a.erun = k.span_words.p + 2 * ns;
    a.epos = k.span_words.p + 3 * ns;
    a.es = k.span_words.p + 4 * ns;
    a.ew = k.span_words.p + 5 * ns;
    a.longs = k.span_words.p + 6 * ns;
    a.kcnt = k.kcnt.p;
    hipLaunchKernelGGL(k_mx_entries, dim3(slot_blocks), blk, 0, s, a);
    hipLaunchKernelGGL(k_mx_pick, dim3(span_blocks), blk, 0, s, a);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (st[kStLong]) hipLaunchKernelGGL(k_mx_pick_wave, dim3(st[kStLong]), dim3(64), 0, s, a);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(4, s));
    hipLaunchKernelGGL(k_mx_keep<false>, dim3(span_blocks), blk, 0, s, a);
    hipLaunchKernelGGL(k_mx_scan, dim3(1), dim3(kScanBlock), 0, s, a.kcnt, a.kcnt, span_blocks,
                       a.status + kStKept);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(st, a.status, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    *n_kept = st[kStKept];
    fits = *n_kept <= cap;
    if (fits && *n_kept) hipLaunchKernelGGL(k_mx_keep<true>, dim3(span_blocks), blk, 0, s, a);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(5, s));
  }
  FS_HIP(hipStreamSynchronize(s));
  for (int j = 0; j < 5; ++j) t_ms[j] = clk.elapsed(j, j + 1);
  t_ms[5] = clk.elapsed(0, ns ? 5 : 3);
  if (!fits) {
    fs_set_error("%llu n-grams need room", (unsigned long long)*n_kept);
    return FS_E_CAPACITY;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_matrix(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                         uint32_t n_script, uint32_t ngram, uint32_t* starts, fs_matrix_ngram* out,
                         uint64_t cap, uint64_t* n_spans, uint64_t* n_kept) {
  bool done = false;
  FS_TRY(mx_check(n_rows, n_script, ngram, out, cap, n_spans, n_kept, &done));
  if (done) {
    if (starts)
      for (uint32_t v = 0; v < n_script; ++v) starts[v] = 0;
    for (double& t : t_ms) t = 0.0;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_starts;
  DBuf<fs_matrix_ngram> d_out;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_starts.reserve(n_script));
  const uint64_t most = n_rows / ngram + 1;                  // n-grams never outnumber this
  FS_TRY(d_out.reserve(cap < most ? cap : most));
  const int rc = mx_run(rows.p, n, n_works, n_script, ngram, d_starts.p, d_out.p, cap, n_spans,
                        n_kept, nullptr);
  if (rc != FS_OK && rc != FS_E_CAPACITY) return rc;
  if (starts && n_script) FS_TRY(copy_out(starts, d_starts, n_script));
  if (rc == FS_OK && *n_kept) FS_TRY(copy_out(out, d_out, *n_kept));
  FS_HIP(hipDeviceSynchronize());
  return rc;
}

extern "C" int fs_matrix_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                              uint32_t n_works, uint32_t n_script, uint32_t ngram,
                              uint32_t* d_starts, fs_matrix_ngram* d_out, uint64_t cap,
                              uint64_t* n_spans, uint64_t* n_kept) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  bool done = false;
  FS_TRY(mx_check(n_rows, n_script, ngram, d_out, cap, n_spans, n_kept, &done));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_starts & 3) ||
      ((uintptr_t)d_out & 3)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_starts and d_out 4-byte");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  if (done) {
    if (d_starts && n_script) {
      FS_HIP(hipMemsetAsync(d_starts, 0, (size_t)n_script * sizeof(uint32_t), ix->stream));
      FS_HIP(hipStreamSynchronize(ix->stream));
    }
    for (double& t : t_ms) t = 0.0;
    return FS_OK;
  }
  return mx_run(d_rows, (uint32_t)n_rows, n_works, n_script, ngram, d_starts, d_out, cap, n_spans,
                n_kept, ix->stream);
}

extern "C" int fs_matrix_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
