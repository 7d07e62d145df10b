// fs_sources.hip -- `ao3.py sources`: which script each fan passage quotes (fs_sources in
// include/fandom_search.h).  K searches of one corpus against K scripts give K lists of
// passages; where passages of different scripts lie on the same fan words they are rivals, and
// a fixed rule says which of them won.  The hot path is an interval join of K sorted lists per
// work: the host's ordering makes every script's list ascending in (work, fan_first) and, since
// the runs of one file do not nest, in (work, fan_last) too, so a passage finds its rivals of a
// script by one binary search and a walk.
//
// Why no schedule changes the result: every value is an integer; adds and maxima commute; the
// outcome is a local maximum of a total order (n_words, n_exact, -script) and asks nothing of
// any other passage's outcome; the best rival is the first of the largest (n_words, n_exact)
// in list order inside a script and the smallest script among equals; a passage's place is a
// count of the passages in front of it, and a row's place a scan of per-work script counts:
// nothing is sorted and nothing comes from arrival.
//
// Separate launches; no workgroup waits on another.  Per file, one after the other:
//   k_src_check    one lane per record: work < n_works
//   (fs_runs_find) the run heads, as fs_passages joins them
//   k_src_seq      one lane per run: kept runs counted per workgroup, then (after k_src_scan)
//                  placed in record order as passage columns, n_exact walked by the lane
// Then, over the lists of all files behind one another:
//   k_src_contest  one lane per (passage, script): a group of `gw` lanes (the power of two at or
//                  above K; 64 under FS_SOURCES_PACK=0) is one passage, a wave 64 / gw of them.
//                  Lane b searches script b's list for the first passage of the work with
//                  fan_last >= p.fan_first and walks it while fan_first <= p.fan_last: rivals,
//                  overlaps, wins and the best key of that script; one more search counts the
//                  passages of script b in front of p.  Segmented wave reductions give the
//                  passage's figures and its place.  The pair figures: up to FS_SOURCES_DENSE
//                  files a workgroup keeps them in LDS over all the passages it strides through
//                  and adds its non-zero entries to the global table, one atomic each; beyond
//                  that every figure is a global atomic.
//   k_src_union    one wave per passage with rivals of two or more scripts (FS_SOURCES_UNION=1:
//                  every contested one): the lanes stride its fan words and test each against
//                  the intersecting range of every rival script by a bounded binary search
//   k_src_has      one lane per passage: the scripts of a work as a 64-bit set (atomic or)
//   k_src_rowscan  one workgroup: a work's first (work, script) row, the scan of the set sizes
//   k_src_rows     one lane per passage: its figures added to its row
//   k_src_works    one lane per work over its row of up to 64 entries: work_scripts, primary,
//                  works_both and the per-script sums, kept in LDS by the workgroup
//   k_src_tables   one lane per script and per pair: the two fixed-size tables
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kMaxK = FS_SOURCES_MAX_FILES;
constexpr uint32_t kMaxPairs = kMaxK * (kMaxK - 1) / 2;
constexpr uint32_t kGroups = 1024;          // workgroups of a pass that keeps figures in LDS
constexpr uint32_t kCols = 9;               // passage columns
// what the FS_SOURCES_MAX_BYTES refusal counts (include/fandom_search.h); a record of the file
// at hand is an fs_row of 32 bytes, with its 28 bytes of columns beside it while it is packed
constexpr uint64_t kRecordBytes = 28, kWorkBytes = 12, kPassageBytes = 160, kRowBytes = 56;

static_assert(sizeof(fs_source_cols) == 40 && sizeof(fs_source_passage) == 80 &&
              sizeof(fs_source_work) == 56 && sizeof(fs_source_script) == 48 &&
              sizeof(fs_source_pair) == 48, "fs_sources");
static_assert(kMaxK == 64, "a work's scripts are one 64-bit set, a passage's lanes one wave");

enum { kStBadRecord = 0, kStSeq = 1, kStWords = 4 };
// per-pair figures of k_src_contest, [figure][pair]
enum { kPContests = 0, kPShared, kPWins, kPFigures };
// per-script sums of k_src_works, [figure][script]
enum { kSWorks = 0, kSPassages, kSAlone, kSWon, kSLost, kSPrimary, kSCovered, kSContested, kSSole,
       kSFigures };

struct SrcArgs {
  uint32_t K, gw, n_works;
  uint32_t off[kMaxK + 1];       // list s is passages off[s] .. off[s + 1]
  uint64_t P;                    // off[K]
  // the passage columns, [P] each
  const uint32_t* scr;
  const uint32_t* work;
  const uint32_t* ff;
  const uint32_t* fl;
  const uint32_t* of;
  const uint32_t* ol;
  const uint32_t* first;
  const uint32_t* nw;
  const uint32_t* nx;
  uint32_t* pos;                 // [P] a passage's place in the merged order
  uint32_t* need;                // [P] 1: contested_words comes from k_src_union
  uint32_t force_union;
  unsigned long long* pair_fig;  // [kPFigures][pairs]
  unsigned long long* has;       // [n_works] the scripts with a passage in the work
  uint32_t* row_of;              // [n_works] the work's first row
  unsigned long long* script_fig;// [kSFigures][K]
  uint32_t* both;                // [pairs] works_both
  fs_source_passage* out;        // [P] in merged order
  fs_source_work* rows;
  fs_source_script* scripts;
  fs_source_pair* pairs;
};

__host__ __device__ inline uint32_t pair_ix(uint32_t a, uint32_t b, uint32_t K) {   // a < b
  return a * (2 * K - a - 1) / 2 + (b - a - 1);
}

__global__ __launch_bounds__(kBlock) void k_src_check(RowsSrc src, uint32_t n, uint32_t n_works,
                                                      uint32_t* status) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool bad = i < n && src.key(i).x >= n_works;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&status[kStBadRecord], 1u);
}

__global__ __launch_bounds__(kScanBlock) void k_src_scan(uint32_t* v, uint32_t n, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(v, n, v, total);
}

// kPlace false: the kept runs of this workgroup's 256 runs into cnt; true: those runs to their
// places as columns [kCols][m] at `cols`, cnt holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_src_seq(RowsSrc src, const uint32_t* heads,
                                                    uint32_t n_runs, uint32_t min_words,
                                                    uint32_t script, uint32_t* cnt, uint32_t* cols,
                                                    uint32_t m) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  uint32_t b = 0, e = 0;
  if (r < n_runs) {
    b = heads[r];
    e = heads[r + 1];
  }
  const bool keep = e - b >= min_words && r < n_runs;
  uint32_t rank, total;
  block_rank<kBlock>(keep, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
  } else if (keep) {
    const size_t p = cnt[blockIdx.x] + rank;
    if (p >= m) return;                               // (never: the counts placed m)
    const uint4 x = src.key(b), y = src.key(e - 1);
    uint32_t exact = 0;
    for (uint32_t i = b; i < e; ++i) exact += src.comb(i) <= 0.0 ? 1u : 0u;
    cols[p] = script;
    cols[(size_t)m + p] = x.x;
    cols[(size_t)2 * m + p] = x.y;
    cols[(size_t)3 * m + p] = y.y;
    cols[(size_t)4 * m + p] = x.z;
    cols[(size_t)5 * m + p] = y.z;
    cols[(size_t)6 * m + p] = b;
    cols[(size_t)7 * m + p] = e - b;
    cols[(size_t)8 * m + p] = exact;
  }
}

// the first j of lo .. hi with (work[j], col[j]) >= (w, x), or > when kAbove; hi without one
template <bool kAbove>
__device__ inline uint32_t src_bound(const uint32_t* work, const uint32_t* col, uint32_t lo,
                                     uint32_t hi, uint32_t w, uint32_t x) {
  const uint64_t key = (uint64_t)w << 32 | x;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint64_t k = (uint64_t)work[mid] << 32 | col[mid];
    if (kAbove ? k <= key : k < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One lane per (passage, script), gw lanes a passage, the workgroup striding through the
// passages.  Dynamic LDS (kDense): kPFigures * pairs 64-bit figures.
template <bool kDense>
__global__ __launch_bounds__(kBlock) void k_src_contest(SrcArgs a) {
  extern __shared__ __align__(16) unsigned long long s_pair[];
  const uint32_t K = a.K, gw = a.gw, n_pairs = K * (K - 1) / 2;
  if (kDense) {
    for (uint32_t i = threadIdx.x; i < kPFigures * n_pairs; i += kBlock) s_pair[i] = 0ull;
    __syncthreads();
  }
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t b = threadIdx.x & (gw - 1);            // this lane's script
  const uint32_t seg = lane & ~(gw - 1);                // the first lane of its passage
  const uint64_t seg_mask = gw == 64 ? ~0ull : ((1ull << gw) - 1);
  const uint32_t per_block = kBlock / gw;
  // every lane of a workgroup goes round the same number of times: `base` is the workgroup's
  for (uint64_t base = (uint64_t)blockIdx.x * per_block; base < a.P;
       base += (uint64_t)gridDim.x * per_block) {
    const uint64_t g = base + threadIdx.x / gw;
    const bool live = g < a.P;
    uint32_t s = 0, w = 0, ff = 0, fl = 0, nw = 0, nx = 0;
    if (live) {
      s = a.scr[g];
      w = a.work[g];
      ff = a.ff[g];
      fl = a.fl[g];
      nw = a.nw[g];
      nx = a.nx[g];
    }
    uint32_t cnt = 0, wins = 0, before = 0, best_nw = 0, best_nx = 0, best_ff = 0;
    uint64_t ov = 0, un = 0;
    if (live && b < K) {
      const uint32_t lo = a.off[b], hi = a.off[b + 1];
      if (b == s) {
        before = (uint32_t)(g - lo);
      } else {
        // of script b in front of p in (work, fan_first, script, first) order
        before = (b < s ? src_bound<true>(a.work, a.ff, lo, hi, w, ff)
                        : src_bound<false>(a.work, a.ff, lo, hi, w, ff)) - lo;
        uint32_t prev_fl = 0;
        for (uint32_t j = src_bound<false>(a.work, a.fl, lo, hi, w, ff);
             j < hi && a.work[j] == w && a.ff[j] <= fl; ++j) {
          const uint32_t qf = a.ff[j], ql = a.fl[j], qw = a.nw[j], qx = a.nx[j];
          const uint32_t from = qf > ff ? qf : ff, to = ql < fl ? ql : fl;
          const uint64_t len = (uint64_t)to - from + 1;
          ov += len;
          // two rivals of one script touch in at most one word: the union counts it once
          un += len - ((cnt && qf == prev_fl && qf >= ff) ? 1u : 0u);
          prev_fl = ql;
          wins += (nw > qw || (nw == qw && (nx > qx || (nx == qx && s < b)))) ? 1u : 0u;
          if (!cnt || qw > best_nw || (qw == best_nw && qx > best_nx)) {
            best_nw = qw;                                // the earliest of the largest: list
            best_nx = qx;                                // order is (fan_first, first) order
            best_ff = qf;
          }
          ++cnt;
        }
        if (cnt && s < b) {
          const uint32_t c = pair_ix(s, b, K);
          if (kDense) {
            atomicAdd(&s_pair[kPContests * n_pairs + c], (unsigned long long)cnt);
            atomicAdd(&s_pair[kPShared * n_pairs + c], (unsigned long long)ov);
            if (wins) atomicAdd(&s_pair[kPWins * n_pairs + c], (unsigned long long)wins);
          } else {
            atomicAdd(&a.pair_fig[(size_t)kPContests * n_pairs + c], (unsigned long long)cnt);
            atomicAdd(&a.pair_fig[(size_t)kPShared * n_pairs + c], (unsigned long long)ov);
            if (wins) atomicAdd(&a.pair_fig[(size_t)kPWins * n_pairs + c], (unsigned long long)wins);
          }
        }
      }
    }
    const uint32_t rivals = seg_sum(cnt, gw);
    const uint32_t rscripts = seg_sum(cnt ? 1u : 0u, gw);
    const uint32_t losses = seg_sum(cnt - wins, gw);
    const uint32_t place = seg_sum(before, gw);
    const uint64_t un_all = seg_sum(un, gw);
    const uint64_t key = cnt ? (uint64_t)best_nw << 32 | best_nx : 0ull;
    const uint64_t top = seg_max(key, gw);
    // the smallest script among the rival scripts whose best passage has the largest key
    const uint64_t cand = (__ballot(cnt && key == top) >> seg) & seg_mask;
    const uint32_t from = seg + (cand ? (uint32_t)__builtin_ctzll(cand) : 0u);
    const uint32_t top_ff = (uint32_t)__shfl((int)best_ff, (int)from);
    if (live && b == 0) {
      const uint64_t span = (uint64_t)fl - ff + 1;
      const bool unite = rscripts >= 2 || (a.force_union && rscripts);
      const uint64_t contested = unite ? 0ull : un_all;
      fs_source_passage o;
      o.script = s;
      o.work = w;
      o.first = a.first[g];
      o.n_words = nw;
      o.n_exact = nx;
      o.fan_first = ff;
      o.fan_last = fl;
      o.orig_first = a.of[g];
      o.orig_last = a.ol[g];
      o.rivals = rivals;
      o.rival_scripts = rscripts;
      o.outcome = !rivals ? FS_SOURCE_ALONE : losses ? FS_SOURCE_LOST : FS_SOURCE_WON;
      o.best_rival = rivals ? from - seg : FS_NONE;
      o.best_rival_words = rivals ? (uint32_t)(top >> 32) : 0u;
      o.best_rival_fan_first = rivals ? top_ff : 0u;
      o.reserved = 0u;
      o.contested_words = contested;
      o.sole_words = span - contested;
      a.pos[g] = place;
      a.need[g] = unite ? 1u : 0u;
      if (place < a.P) a.out[place] = o;                // (always: place counts passages)
    }
  }
  if (!kDense) return;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kPFigures * n_pairs; i += kBlock)
    if (s_pair[i]) atomicAdd(&a.pair_fig[i], s_pair[i]);
}

// One wave per passage that needs it: the words of its span inside a rival's.
__global__ __launch_bounds__(kBlock) void k_src_union(SrcArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t g = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (g >= a.P || !a.need[g]) return;                   // wave-uniform
  const uint32_t s = a.scr[g], w = a.work[g], ff = a.ff[g], fl = a.fl[g];
  uint32_t lo = 0, cnt = 0;
  if (lane < a.K && lane != s) {
    const uint32_t l0 = a.off[lane], h0 = a.off[lane + 1];
    lo = src_bound<false>(a.work, a.fl, l0, h0, w, ff);
    const uint32_t hi = src_bound<true>(a.work, a.ff, lo, h0, w, fl);
    cnt = hi - lo;
  }
  const uint64_t rival = __ballot(cnt != 0);
  uint64_t covered = 0;
  for (uint64_t x0 = ff; x0 <= fl; x0 += 64) {
    const uint64_t x = x0 + lane;
    bool in = false;
    for (uint64_t m = rival; m; m &= m - 1) {
      const uint32_t bb = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
      const uint32_t l = lane_u32(lo, bb), h = l + lane_u32(cnt, bb);
      if (x <= fl && !in) {
        const uint32_t j = src_bound<false>(a.work, a.fl, l, h, w, (uint32_t)x);
        in = j < h && a.ff[j] <= (uint32_t)x;
      }
    }
    covered += (uint64_t)__popcll(__ballot(in));
  }
  if (lane == 0 && a.pos[g] < a.P) {
    fs_source_passage* o = &a.out[a.pos[g]];
    o->contested_words = covered;
    o->sole_words = (uint64_t)fl - ff + 1 - covered;
  }
}

__global__ __launch_bounds__(kBlock) void k_src_has(SrcArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.P) return;
  const uint32_t s = a.scr[g], w = a.work[g];
  if (g == a.off[s] || a.work[g - 1] != w) atomicOr(&a.has[w], 1ull << s);
}

__global__ __launch_bounds__(kScanBlock) void k_src_rowscan(SrcArgs a, unsigned long long* total) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  const unsigned long long* has = a.has;
  uint32_t* row_of = a.row_of;
  const uint64_t sum = scan_chunks<1, uint32_t, uint64_t>(
      a.n_works, [has](uint64_t j) { return (uint32_t)__popcll(has[j]); },
      [row_of](uint64_t j, uint64_t pre, uint32_t) { row_of[j] = (uint32_t)pre; }, s_w);
  if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kBlock) void k_src_rows(SrcArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.P) return;
  const uint32_t s = a.scr[g], w = a.work[g];
  if (a.pos[g] >= a.P) return;                          // (never: a place counts passages)
  const fs_source_passage* o = &a.out[a.pos[g]];
  fs_source_work* r = &a.rows[a.row_of[w] + (uint32_t)__popcll(a.has[w] & ((1ull << s) - 1))];
  atomicAdd(&r->passages, 1u);
  const uint32_t oc = o->outcome;
  atomicAdd(oc == FS_SOURCE_ALONE ? &r->alone : oc == FS_SOURCE_WON ? &r->won : &r->lost, 1u);
  atomicAdd((unsigned long long*)&r->covered_words,
            (unsigned long long)(o->contested_words + o->sole_words));
  if (o->contested_words)
    atomicAdd((unsigned long long*)&r->contested_words, (unsigned long long)o->contested_words);
  if (o->sole_words)
    atomicAdd((unsigned long long*)&r->sole_words, (unsigned long long)o->sole_words);
}

// One lane per work, the workgroup striding through the works; the per-script sums and
// works_both in LDS until the end.
__global__ __launch_bounds__(kBlock) void k_src_works(SrcArgs a) {
  __shared__ unsigned long long s_fig[kSFigures * kMaxK];
  __shared__ uint32_t s_both[kMaxPairs];
  const uint32_t K = a.K, n_pairs = K * (K - 1) / 2;
  for (uint32_t i = threadIdx.x; i < kSFigures * K; i += kBlock) s_fig[i] = 0ull;
  for (uint32_t i = threadIdx.x; i < n_pairs; i += kBlock) s_both[i] = 0u;
  __syncthreads();
  for (uint64_t w = (uint64_t)blockIdx.x * kBlock + threadIdx.x; w < a.n_works;
       w += (uint64_t)gridDim.x * kBlock) {
    const uint64_t has = a.has[w];
    if (!has) continue;
    fs_source_work* r = a.rows + a.row_of[w];
    const uint32_t n = (uint32_t)__popcll(has);
    uint32_t primary = 0, k = 0;
    uint64_t most = 0;
    for (uint64_t m = has; m; m &= m - 1, ++k)          // ascending script: a tie keeps the smaller
      if (!k || r[k].covered_words > most) {
        most = r[k].covered_words;
        primary = k;
      }
    k = 0;
    for (uint64_t m = has; m; m &= m - 1, ++k) {
      const uint32_t s = (uint32_t)__builtin_ctzll(m);
      r[k].work = (uint32_t)w;
      r[k].script = s;
      r[k].work_scripts = n;
      r[k].primary = k == primary ? 1u : 0u;
      atomicAdd(&s_fig[kSWorks * K + s], 1ull);
      atomicAdd(&s_fig[kSPassages * K + s], (unsigned long long)r[k].passages);
      atomicAdd(&s_fig[kSAlone * K + s], (unsigned long long)r[k].alone);
      atomicAdd(&s_fig[kSWon * K + s], (unsigned long long)r[k].won);
      atomicAdd(&s_fig[kSLost * K + s], (unsigned long long)r[k].lost);
      if (k == primary) atomicAdd(&s_fig[kSPrimary * K + s], 1ull);
      atomicAdd(&s_fig[kSCovered * K + s], (unsigned long long)r[k].covered_words);
      atomicAdd(&s_fig[kSContested * K + s], (unsigned long long)r[k].contested_words);
      atomicAdd(&s_fig[kSSole * K + s], (unsigned long long)r[k].sole_words);
      for (uint64_t m2 = m & (m - 1); m2; m2 &= m2 - 1)
        atomicAdd(&s_both[pair_ix(s, (uint32_t)__builtin_ctzll(m2), K)], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kSFigures * K; i += kBlock)
    if (s_fig[i]) atomicAdd(&a.script_fig[i], s_fig[i]);
  for (uint32_t i = threadIdx.x; i < n_pairs; i += kBlock)
    if (s_both[i]) atomicAdd(&a.both[i], s_both[i]);
}

__global__ __launch_bounds__(kBlock) void k_src_tables(SrcArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t K = a.K, n_pairs = K * (K - 1) / 2;
  if (i < K) {
    const unsigned long long* f = a.script_fig;
    a.scripts[i] = fs_source_script{(uint32_t)f[kSWorks * K + i],  (uint32_t)f[kSPassages * K + i],
                                    (uint32_t)f[kSAlone * K + i],  (uint32_t)f[kSWon * K + i],
                                    (uint32_t)f[kSLost * K + i],   (uint32_t)f[kSPrimary * K + i],
                                    f[kSCovered * K + i],          f[kSContested * K + i],
                                    f[kSSole * K + i]};
  }
  if (i < n_pairs) {
    uint32_t p = 0, q = 0;                              // pair i is (p, q)
    for (uint32_t rest = i; rest >= K - p - 1; ++p) rest -= K - p - 1;
    q = p + 1 + (i - pair_ix(p, p + 1, K));
    const uint64_t c = a.pair_fig[kPContests * n_pairs + i], v = a.pair_fig[kPWins * n_pairs + i];
    a.pairs[i] = fs_source_pair{p, q, a.both[i], 0u, c, a.pair_fig[kPShared * n_pairs + i], v, c - v};
  }
}

thread_local double t_ms[5];    // passages, contest, union, rollups, total of the last call

// tables of a call without a passage
void src_none(uint32_t K, fs_source_script* scripts, fs_source_pair* pairs) {
  for (uint32_t s = 0; s < K; ++s) scripts[s] = fs_source_script{0u, 0u, 0u, 0u, 0u, 0u, 0ull, 0ull, 0ull};
  for (uint32_t p = 0; p < K; ++p)
    for (uint32_t q = p + 1; q < K; ++q)
      pairs[pair_ix(p, q, K)] = fs_source_pair{p, q, 0u, 0u, 0ull, 0ull, 0ull, 0ull};
}

struct RunsHold {
  fs_runs* r = nullptr;
  ~RunsHold() { if (r) fs_runs_free(r); }
};

}  // namespace

extern "C" int fs_sources(int device, const fs_source_cols* files, uint32_t n_files,
                          uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                          fs_source_passage* passages, uint64_t cap_passages,
                          uint64_t* n_passages, fs_source_work* works, uint64_t cap_works,
                          uint64_t* n_work_rows, fs_source_script* scripts,
                          fs_source_pair* pairs) {
  const uint32_t K = n_files;
  if (K > kMaxK) {
    fs_set_error("%u files: sources take up to %u", K, kMaxK);
    return FS_E_UNSUPPORTED;
  }
  if (!K || !files || !n_passages || !n_work_rows || !scripts || (K > 1 && !pairs) ||
      (cap_passages && !passages) || (cap_works && !works)) {
    fs_set_error(K ? "null argument" : "no files");
    return FS_E_INVALID;
  }
  uint64_t n_max = 0;
  for (uint32_t s = 0; s < K; ++s) {
    if (files[s].n >= (1ull << 32)) {
      fs_set_error("file %u has %llu records: sources take fewer than 2^32 each", s,
                   (unsigned long long)files[s].n);
      return FS_E_UNSUPPORTED;
    }
    if (files[s].n > n_max) n_max = files[s].n;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  const uint64_t fixed = kRecordBytes * n_max + kWorkBytes * n_works;
  if (fixed > FS_SOURCES_MAX_BYTES) {
    fs_set_error("%llu bytes of device tables: sources take up to %llu",
                 (unsigned long long)fixed, (unsigned long long)FS_SOURCES_MAX_BYTES);
    return FS_E_UNSUPPORTED;
  }
  for (uint32_t s = 0; s < K; ++s)
    if (files[s].n && (!files[s].work || !files[s].fan_ix || !files[s].orig_ix || !files[s].comb)) {
      fs_set_error("null argument");
      return FS_E_INVALID;
    }
  *n_passages = 0;
  *n_work_rows = 0;
  for (double& t : t_ms) t = 0.0;
  if (!n_max) {
    src_none(K, scripts, pairs);
    return FS_OK;
  }
  if (!n_works) {
    fs_set_error("a work >= n_works (0)");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  hipStream_t st = nullptr;
  const dim3 blk(kBlock);
  Clock<5> clk;
  SrcArgs a{};
  a.K = K;
  a.n_works = n_works;
  DBuf<uint32_t> status, cnt;
  DBuf<fs_row> rows;
  std::vector<DBuf<uint32_t>> part(K);
  FS_TRY(status.reserve(kStWords));
  FS_TRY(clk.mark(0, st));

  // the passage columns, file by file
  for (uint32_t s = 0; s < K; ++s) {
    const uint32_t n = (uint32_t)files[s].n;
    a.off[s + 1] = a.off[s];
    if (!n) continue;
    FS_TRY(fs_host_rows(rows, files[s].work, files[s].fan_ix, files[s].orig_ix, n, nullptr,
                        files[s].comb));
    const RowsSrc src{rows.p};
    FS_HIP(hipMemsetAsync(status.p, 0, kStWords * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_src_check, dim3(blocks_of(n, kBlock)), blk, 0, st, src, n, n_works,
                       status.p);
    FS_HIP(hipGetLastError());
    RunsHold runs;
    const uint32_t* heads = nullptr;
    uint32_t n_runs = 0;
    const int rc = fs_runs_find(rows.p, n, min_words, max_gap, st, &runs.r, &heads, &n_runs);
    if (rc != FS_OK) {
      if (rc == FS_E_INVALID) fs_set_error("file %u: records are not sorted by (work, fan_ix)", s);
      return rc;
    }
    const uint32_t run_blocks = blocks_of(n_runs, kBlock);
    FS_TRY(cnt.reserve(run_blocks));
    if (run_blocks)
      hipLaunchKernelGGL(k_src_seq<false>, dim3(run_blocks), blk, 0, st, src, heads, n_runs,
                         min_words, s, cnt.p, (uint32_t*)nullptr, 0u);
    hipLaunchKernelGGL(k_src_scan, dim3(1), dim3(kScanBlock), 0, st, cnt.p, run_blocks,
                       status.p + kStSeq);
    FS_HIP(hipGetLastError());
    uint32_t h[kStWords];
    FS_HIP(hipMemcpyAsync(h, status.p, sizeof h, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    if (h[kStBadRecord]) {
      fs_set_error("file %u: a work >= n_works (%u)", s, n_works);
      return FS_E_INVALID;
    }
    const uint32_t m = h[kStSeq];
    const uint64_t total = (uint64_t)a.off[s] + m;
    if (fixed + kPassageBytes * total > FS_SOURCES_MAX_BYTES) {
      fs_set_error("%llu passages: their tables pass %llu bytes", (unsigned long long)total,
                   (unsigned long long)FS_SOURCES_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    a.off[s + 1] = (uint32_t)total;
    if (!m) continue;
    FS_TRY(part[s].reserve((size_t)kCols * m));
    hipLaunchKernelGGL(k_src_seq<true>, dim3(run_blocks), blk, 0, st, src, heads, n_runs,
                       min_words, s, cnt.p, part[s].p, m);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(st));                   // the records go before the next file's
  }
  const uint64_t P = a.off[K];
  a.P = P;
  *n_passages = P;
  if (!P) {
    src_none(K, scripts, pairs);
    FS_TRY(clk.mark(1, st));
    FS_HIP(hipStreamSynchronize(st));
    t_ms[0] = t_ms[4] = clk.elapsed(0, 1);
    return FS_OK;
  }
  DBuf<uint32_t> cols, misc, both;
  FS_TRY(cols.reserve((size_t)kCols * P));
  for (uint32_t s = 0; s < K; ++s) {
    const size_t m = a.off[s + 1] - a.off[s];
    for (uint32_t c = 0; c < kCols && m; ++c)
      FS_HIP(hipMemcpyAsync(cols.p + (size_t)c * P + a.off[s], part[s].p + (size_t)c * m,
                            m * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  }
  a.scr = cols.p;
  a.work = cols.p + P;
  a.ff = cols.p + 2 * P;
  a.fl = cols.p + 3 * P;
  a.of = cols.p + 4 * P;
  a.ol = cols.p + 5 * P;
  a.first = cols.p + 6 * P;
  a.nw = cols.p + 7 * P;
  a.nx = cols.p + 8 * P;
  FS_TRY(clk.mark(1, st));

  // the contests
  const uint32_t n_pairs = K * (K - 1) / 2;
  uint32_t gw = 1;
  while (gw < K) gw <<= 1;
  if (!env_u32("FS_SOURCES_PACK", 1, 1)) gw = 64;
  a.gw = gw;
  a.force_union = env_u32("FS_SOURCES_UNION", 0, 1);
  const bool dense = K <= env_u32("FS_SOURCES_DENSE", kMaxK, kMaxK);
  DBuf<unsigned long long> fig, has;
  DBuf<fs_source_passage> d_out;
  FS_TRY(misc.reserve(2 * P + n_works));
  FS_TRY(fig.reserve((size_t)kPFigures * n_pairs + (size_t)kSFigures * K));
  FS_TRY(has.reserve(n_works));
  FS_TRY(both.reserve(n_pairs));
  FS_TRY(d_out.reserve(P));
  a.pos = misc.p;
  a.need = misc.p + P;
  a.row_of = misc.p + 2 * P;
  a.pair_fig = fig.p;
  a.script_fig = fig.p + (size_t)kPFigures * n_pairs;
  a.has = has.p;
  a.both = both.p;
  a.out = d_out.p;
  FS_HIP(hipMemsetAsync(fig.p, 0, ((size_t)kPFigures * n_pairs + (size_t)kSFigures * K) * 8, st));
  FS_HIP(hipMemsetAsync(has.p, 0, (size_t)n_works * 8, st));
  FS_HIP(hipMemsetAsync(both.p, 0, (n_pairs ? n_pairs : 1) * sizeof(uint32_t), st));
  const uint32_t groups = blocks_of(P, kBlock / gw);
  if (dense)
    hipLaunchKernelGGL(k_src_contest<true>, dim3(groups < kGroups ? groups : kGroups), blk,
                       (size_t)kPFigures * n_pairs * 8, st, a);
  else
    hipLaunchKernelGGL(k_src_contest<false>, dim3(groups < kGroups ? groups : kGroups), blk, 0,
                       st, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(2, st));
  hipLaunchKernelGGL(k_src_union, dim3(blocks_of(P, kBlock / 64)), blk, 0, st, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(3, st));

  // the rollups
  DBuf<unsigned long long> d_total;
  DBuf<fs_source_work> d_rows;
  DBuf<fs_source_script> d_scripts;
  DBuf<fs_source_pair> d_pairs;
  FS_TRY(d_total.reserve(1));
  FS_TRY(d_scripts.reserve(K));
  FS_TRY(d_pairs.reserve(n_pairs));
  a.scripts = d_scripts.p;
  a.pairs = d_pairs.p;
  hipLaunchKernelGGL(k_src_has, dim3(blocks_of(P, kBlock)), blk, 0, st, a);
  hipLaunchKernelGGL(k_src_rowscan, dim3(1), dim3(kScanBlock), 0, st, a, d_total.p);
  FS_HIP(hipGetLastError());
  unsigned long long R = 0;
  FS_HIP(hipMemcpyAsync(&R, d_total.p, sizeof R, hipMemcpyDeviceToHost, st));
  FS_HIP(hipStreamSynchronize(st));
  *n_work_rows = R;
  if (fixed + kPassageBytes * P + kRowBytes * R > FS_SOURCES_MAX_BYTES) {
    fs_set_error("%llu passages and %llu rows: their tables pass %llu bytes",
                 (unsigned long long)P, R, (unsigned long long)FS_SOURCES_MAX_BYTES);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(d_rows.reserve(R));
  a.rows = d_rows.p;
  FS_HIP(hipMemsetAsync(d_rows.p, 0, (size_t)R * sizeof(fs_source_work), st));
  const uint32_t work_blocks = blocks_of(n_works, kBlock);
  hipLaunchKernelGGL(k_src_rows, dim3(blocks_of(P, kBlock)), blk, 0, st, a);
  hipLaunchKernelGGL(k_src_works, dim3(work_blocks < kGroups ? work_blocks : kGroups), blk, 0, st,
                     a);
  hipLaunchKernelGGL(k_src_tables, dim3(blocks_of(n_pairs > K ? n_pairs : K, kBlock)), blk, 0, st,
                     a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, st));
  FS_HIP(hipMemcpyAsync(scripts, d_scripts.p, (size_t)K * sizeof(fs_source_script),
                        hipMemcpyDeviceToHost, st));
  if (n_pairs)
    FS_HIP(hipMemcpyAsync(pairs, d_pairs.p, (size_t)n_pairs * sizeof(fs_source_pair),
                          hipMemcpyDeviceToHost, st));
  const bool fits = P <= cap_passages && R <= cap_works;
  if (fits) {
    FS_HIP(hipMemcpyAsync(passages, d_out.p, (size_t)P * sizeof(fs_source_passage),
                          hipMemcpyDeviceToHost, st));
    FS_HIP(hipMemcpyAsync(works, d_rows.p, (size_t)R * sizeof(fs_source_work),
                          hipMemcpyDeviceToHost, st));
  }
  FS_HIP(hipStreamSynchronize(st));
  for (int j = 0; j < 4; ++j) t_ms[j] = clk.elapsed(j, j + 1);
  t_ms[4] = clk.elapsed(0, 4);
  if (!fits) {
    fs_set_error("%llu passages and %llu rows need room", (unsigned long long)P, R);
    return FS_E_CAPACITY;
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_sources_times(double* ms) {
  return times_out(ms, t_ms, 5);
}
