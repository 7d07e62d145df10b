// fs_quotes.hip -- `ao3.py quotes`: match records sorted by (work, fan_ix) seen from the
// script's side (fs_quotes, fs_quotes_rows in include/fandom_search.h): per script word its
// records, the distinct works behind them, the passages covering it and the distinct works
// behind those (its depth); and the regions, maximal stretches of depth >= min_works, with
// their passages, works, sums and peak.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   fs_runs_find       the run heads of fs_passages.hip (and its sortedness check)
//   k_quotes_runs      one lane per run: work boundaries; a passage's span as +1 / -1 in a
//                      difference array over the script, +1 in an array of span starts
//   k_quotes_slices<0> works of more than `slice` records: a wave per slice of records reduces
//                      its part in LDS (bit per script word) and merges it into the work's
//                      global bitmap; the bits atomicOr finds clear are the words this work
//                      reaches first.  The spans of its passages go straight to a second
//                      global bitmap, a word of bits at a time
//   k_quotes_each<0>   a wave per work (per kWorksPerWave works when they are many) of at most
//                      `slice` records: both bitmaps in LDS
//   k_quotes_scan      one workgroup over the script: passages per word, span starts up to a
//                      word, region heads up to a word, the word's region
//   k_quotes_fill      one lane per script word: a region's first and last word
//   k_quotes_reduce    one lane per region (the wave for a long one): sums, peak and its run,
//                      passages from the scanned span starts
//   k_quotes_slices<1>, k_quotes_each<1>   the same bitmap per work over region ids: a span
//                      is a contiguous range of them; distinct works per region
// A workgroup is one wave with its own LDS, sized from n_script (two bits per script word at
// most: 128 KB at FS_WORKS_MAX_SCRIPT, of the CU's 160 KB) or from the number of regions.
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kSlice = 8192;          // records per slice of a large work, at least (quotes_run)
constexpr uint32_t kWorksPerWave = 8;       // works a wave takes when there are many (quotes_run)
constexpr uint32_t kDepth = 4;              // chunks of 64 records whose loads are in flight together
constexpr uint32_t kScanItems = 4;          // script words per thread of the one-workgroup scan
constexpr uint32_t kRunBlock = 256;
constexpr uint32_t kLong = 256;             // regions of this many words are reduced by a wave
constexpr size_t kLdsMax = 160 * 1024;      // LDS of a CU

constexpr uint32_t kWordU32 = sizeof(fs_quote_word) / 4;       // counters of a word, as uint32
constexpr uint32_t kRegionU32 = sizeof(fs_quote_region) / 4;
// positions of the counters the kernels add to
constexpr uint32_t kWNWords = 0, kWNExact = 1, kWNWorks = 2, kWNPassageWorks = 4;
constexpr uint32_t kRNWorks = 3;
static_assert(offsetof(fs_quote_word, n_words) == 4 * kWNWords, "fs_quote_word");
static_assert(offsetof(fs_quote_word, n_exact) == 4 * kWNExact, "fs_quote_word");
static_assert(offsetof(fs_quote_word, n_works) == 4 * kWNWorks, "fs_quote_word");
static_assert(offsetof(fs_quote_word, n_passage_works) == 4 * kWNPassageWorks, "fs_quote_word");
static_assert(offsetof(fs_quote_region, n_works) == 4 * kRNWorks, "fs_quote_region");

struct QuotesArgs {
  uint32_t n, n_works, n_script, bw, n_regions, rbw, slice, min_words, min_works, per_wave, n_runs;
  const uint32_t* heads;        // [n_runs + 1] first record of a run
  uint32_t* wstart;             // [n_works] first record of a work
  uint32_t* wend;               // [n_works] one past its last (both 0: no records)
  uint32_t* diff;               // [n_script + 1] +1 at a span's first word, -1 behind its last
  uint32_t* starts;             // [n_script] spans that start at a word
  uint32_t* s0;                 // [n_script] spans that start at or before a word
  uint32_t* hc;                 // [n_script] region heads at or before a word
  uint32_t* area;               // [tiles][2 * bw] merge areas of large works: records, spans
  uint32_t* rarea;              // [tiles][rbw] ... over region ids
  uint32_t* status;             // [0] invalid input, [1] regions
  fs_quote_word* words;
  fs_quote_region* regions;
};

// one lane per run
__global__ __launch_bounds__(kRunBlock) void k_quotes_runs(RowsSrc src, QuotesArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  bool bad = false;
  if (r < a.n_runs) {
    const uint32_t h = a.heads[r], e = a.heads[r + 1];
    const uint4 k = src.key(h);
    const uint32_t w = k.x;
    if (w >= a.n_works) {
      bad = true;
    } else {
      const uint32_t pw = h ? src.key(h - 1).x : FS_NONE;
      if (pw != w) {
        a.wstart[w] = h;
        if (h && pw < a.n_works) a.wend[pw] = h;
      }
      if (r + 1 == a.n_runs) a.wend[w] = a.n;
      if (e - h >= a.min_words) {
        const uint32_t o0 = k.z, o1 = src.key((uint64_t)e - 1).z;    // o0 <= o1: a run steps forward
        if (o1 >= a.n_script) {
          bad = true;
        } else {
          atomicAdd(&a.diff[o0], 1u);
          atomicAdd(&a.diff[o1 + 1], 0xFFFFFFFFu);
          atomicAdd(&a.starts[o0], 1u);
        }
      }
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
}

// first run whose head is at or behind record i (wave-uniform)
__device__ inline uint32_t run_from(const QuotesArgs& a, uint64_t i) {
  uint32_t lo = 0, hi = a.n_runs;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.heads[mid] < i) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// What a kept run covers, as an inclusive range of bits: script words (kLevel 0), or the ids of
// the regions its span intersects (kLevel 1: contiguous; none when lo > hi).
template <int kLevel>
__device__ inline bool run_range(const RowsSrc& src, const QuotesArgs& a, uint32_t r, int64_t* lo,
                                 int64_t* hi) {
  const uint32_t h = a.heads[r], e = a.heads[r + 1];
  if (e - h < a.min_words) return false;
  const uint32_t o0 = src.key(h).z, o1 = src.key((uint64_t)e - 1).z;
  if (o1 >= a.n_script) return false;               // (flagged by k_quotes_runs)
  if (kLevel == 0) {
    *lo = o0;
    *hi = o1;
  } else {
    const uint32_t c0 = a.hc[o0];
    *lo = a.words[o0].region != FS_NONE ? (int64_t)c0 - 1 : (int64_t)c0;
    *hi = (int64_t)a.hc[o1] - 1;
  }
  return *lo <= *hi;
}

// The ranges of runs [rs, re) into the bitmap `bm` (LDS or a global merge area), a word of bits
// at a time, one lane per run; every bit found clear adds 1 to its counter cnt[bit * stride].
template <int kLevel>
__device__ inline void mark_runs(const RowsSrc& src, const QuotesArgs& a, uint32_t rs, uint32_t re,
                                 uint32_t* bm, uint32_t* cnt, uint32_t stride) {
  for (uint64_t r = (uint64_t)rs + threadIdx.x; r < re; r += kWave) {
    int64_t lo, hi;
    if (!run_range<kLevel>(src, a, (uint32_t)r, &lo, &hi)) continue;
    const uint32_t k0 = (uint32_t)(lo >> 5), k1 = (uint32_t)(hi >> 5);
    for (uint32_t k = k0; k <= k1; ++k) {
      uint32_t m = 0xFFFFFFFFu;
      if (k == k0) m &= 0xFFFFFFFFu << (lo & 31);
      if (k == k1) m &= 0xFFFFFFFFu >> (31 - (hi & 31));
      for (uint32_t nb = m & ~atomicOr(&bm[k], m); nb; nb &= nb - 1)
        atomicAdd(&cnt[(size_t)(k * 32 + (uint32_t)__builtin_ctz(nb)) * stride], 1u);
    }
  }
}

// the bitmap words those runs touched, cleared again
template <int kLevel>
__device__ inline void unmark_runs(const RowsSrc& src, const QuotesArgs& a, uint32_t rs,
                                   uint32_t re, uint32_t* bm) {
  for (uint64_t r = (uint64_t)rs + threadIdx.x; r < re; r += kWave) {
    int64_t lo, hi;
    if (!run_range<kLevel>(src, a, (uint32_t)r, &lo, &hi)) continue;
    for (uint32_t k = (uint32_t)(lo >> 5); k <= (uint32_t)(hi >> 5); ++k) bm[k] = 0;
  }
}

// Records [b, e) (wave-uniform) into the LDS bitmap `bm`: n_words and n_exact of their script
// words by atomics.  kFirst: a bit found clear adds 1 to the word's n_works (a work of one
// wave); otherwise the bitmap is merged afterwards.  *bad |= an orig_ix outside the script.
template <bool kFirst>
__device__ inline void add_records(const RowsSrc& src, const QuotesArgs& a, uint32_t* bm,
                                   uint64_t b, uint64_t e, bool* bad) {
  uint32_t* __restrict__ cnt = reinterpret_cast<uint32_t*>(a.words);
  for (uint64_t c = b; c < e; c += kDepth * kWave) {
    uint32_t os[kDepth];
    double vs[kDepth];
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {           // the loads of kDepth chunks in flight
      const uint64_t i = c + u * kWave + threadIdx.x;
      os[u] = i < e ? src.key(i).z : 0u;
      vs[u] = i < e ? src.comb(i) : __builtin_nan("");
    }
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {
      const uint64_t i = c + u * kWave + threadIdx.x;
      if (i >= e) continue;
      const uint32_t o = os[u];
      if (o >= a.n_script) {
        *bad = true;
        continue;
      }
      const uint32_t bit = 1u << (o & 31);
      const bool first = !(atomicOr(&bm[o >> 5], bit) & bit);
      uint32_t* __restrict__ w = cnt + (size_t)o * kWordU32;
      atomicAdd(&w[kWNWords], 1u);
      if (vs[u] <= 0.0) atomicAdd(&w[kWNExact], 1u);
      if (kFirst && first) atomicAdd(&w[kWNWorks], 1u);
    }
  }
}

extern __shared__ uint32_t s_quotes[];

// a wave per slice of records: the parts of large works inside it
template <int kLevel>
__global__ __launch_bounds__(kWave) void k_quotes_slices(RowsSrc src, QuotesArgs a) {
  const uint32_t lane = threadIdx.x;
  if (kLevel == 0) {
    for (uint32_t k = lane; k < a.bw; k += kWave) s_quotes[k] = 0;
    __syncthreads();
  }
  const uint64_t t0 = (uint64_t)blockIdx.x * a.slice;
  const uint64_t t1 = t0 + a.slice < a.n ? t0 + a.slice : a.n;
  // only the works of the first and the last record can have more records than the slice
  const uint32_t wa = src.key(t0).x, wb = src.key(t1 - 1).x;
  bool bad = false;
  for (int pass = 0; pass < 2; ++pass) {
    const uint32_t w = pass ? wb : wa;
    if ((pass && wb == wa) || w >= a.n_works) continue;
    const uint32_t ws = a.wstart[w], we = a.wend[w];
    if (we - ws <= a.slice) continue;
    const uint64_t b = ws > t0 ? ws : t0, e = we < t1 ? we : t1;
    const uint32_t rs = run_from(a, b), re = run_from(a, e);   // runs whose head is in [b, e)
    if (kLevel == 0) {
      uint32_t* __restrict__ g = a.area + (size_t)(ws / a.slice) * 2 * a.bw;
      add_records<false>(src, a, s_quotes, b, e, &bad);
      __syncthreads();
      uint32_t* __restrict__ cnt = reinterpret_cast<uint32_t*>(a.words);
      for (uint32_t k = lane; k < a.bw; k += kWave) {
        const uint32_t v = s_quotes[k];
        if (!v) continue;
        s_quotes[k] = 0;
        for (uint32_t nb = v & ~atomicOr(&g[k], v); nb; nb &= nb - 1)
          atomicAdd(&cnt[(size_t)(k * 32 + (uint32_t)__builtin_ctz(nb)) * kWordU32 + kWNWorks], 1u);
      }
      mark_runs<0>(src, a, rs, re, g + a.bw, cnt + kWNPassageWorks, kWordU32);
      __syncthreads();
    } else {
      mark_runs<1>(src, a, rs, re, a.rarea + (size_t)(ws / a.slice) * a.rbw,
                        reinterpret_cast<uint32_t*>(a.regions) + kRNWorks, kRegionU32);
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
}

// a wave per a.per_wave works
template <int kLevel>
__global__ __launch_bounds__(kWave) void k_quotes_each(RowsSrc src, QuotesArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint32_t lds_words = kLevel ? a.rbw : 2 * a.bw;
  for (uint32_t k = lane; k < lds_words; k += kWave) s_quotes[k] = 0;
  __syncthreads();
  const uint64_t w0 = (uint64_t)blockIdx.x * a.per_wave;
  const uint64_t w1 = w0 + a.per_wave < a.n_works ? w0 + a.per_wave : a.n_works;
  bool bad = false;
  for (uint64_t w = w0; w < w1; ++w) {
    const uint32_t ws = a.wstart[w], we = a.wend[w], nw = we - ws;
    if (nw == 0 || nw > a.slice) continue;           // none, or k_quotes_slices' work
    const uint32_t rs = run_from(a, ws), re = run_from(a, we);
    if (kLevel == 0) {
      add_records<true>(src, a, s_quotes, ws, we, &bad);
      mark_runs<0>(src, a, rs, re, s_quotes + a.bw,
                        reinterpret_cast<uint32_t*>(a.words) + kWNPassageWorks, kWordU32);
    } else {
      mark_runs<1>(src, a, rs, re, s_quotes,
                        reinterpret_cast<uint32_t*>(a.regions) + kRNWorks, kRegionU32);
    }
    if (w + 1 == w1) break;
    __syncthreads();
    if (kLevel == 0) {
      for (uint64_t i = (uint64_t)ws + lane; i < we; i += kWave) {
        const uint32_t o = src.key(i).z;
        if (o < a.n_script) s_quotes[o >> 5] = 0;
      }
      unmark_runs<0>(src, a, rs, re, s_quotes + a.bw);
    } else {
      unmark_runs<1>(src, a, rs, re, s_quotes);
    }
    __syncthreads();
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
}

// One workgroup over the script, chunks of 4096 words in turn: per word the passages covering
// it (scan of diff), the spans starting at or before it, the region heads at or before it and
// its region; status[1] = regions.
__global__ __launch_bounds__(kScanBlock) void k_quotes_scan(QuotesArgs a) {
  __shared__ uint32_t s_w[3][kScanBlock / 64];
  uint32_t carry_p = 0, carry_s = 0, carry_h = 0;
  for (uint64_t c = 0; c < a.n_script; c += kScanBlock * kScanItems) {
    const uint64_t j0 = c + (uint64_t)threadIdx.x * kScanItems;
    uint32_t p[kScanItems], s[kScanItems], h[kScanItems];
    bool in[kScanItems];
    uint32_t mp = 0, ms = 0, mh = 0;
    bool before = j0 > 0 && j0 - 1 < a.n_script && a.words[j0 - 1].n_passage_works >= a.min_works;
#pragma unroll
    for (uint32_t t = 0; t < kScanItems; ++t) {
      const uint64_t j = j0 + t;
      p[t] = s[t] = h[t] = 0;
      in[t] = false;
      if (j < a.n_script) {
        p[t] = a.diff[j];
        s[t] = a.starts[j];
        in[t] = a.words[j].n_passage_works >= a.min_works;
        h[t] = in[t] && !before ? 1u : 0u;
        before = in[t];
      }
      mp += p[t];
      ms += s[t];
      mh += h[t];
    }
    uint32_t tp, ts, th;
    uint32_t ap = carry_p + block_scan<kScanBlock>(mp, s_w[0], &tp);
    uint32_t as = carry_s + block_scan<kScanBlock>(ms, s_w[1], &ts);
    uint32_t ah = carry_h + block_scan<kScanBlock>(mh, s_w[2], &th);
#pragma unroll
    for (uint32_t t = 0; t < kScanItems; ++t) {
      const uint64_t j = j0 + t;
      ap += p[t];
      as += s[t];
      ah += h[t];
      if (j < a.n_script) {
        a.words[j].n_passages = ap;
        a.words[j].region = in[t] ? ah - 1 : FS_NONE;
        a.s0[j] = as;
        a.hc[j] = ah;
      }
    }
    carry_p += tp;
    carry_s += ts;
    carry_h += th;
  }
  if (threadIdx.x == 0) a.status[1] = carry_h;
}

// words without records (n_rows == 0)
__global__ __launch_bounds__(kRunBlock) void k_quotes_none(fs_quote_word* __restrict__ words,
                                                           uint32_t n_script) {
  const uint64_t j = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (j >= n_script) return;
  fs_quote_word w{};
  w.region = FS_NONE;
  words[j] = w;
}

// one lane per script word: the ends of its region
__global__ __launch_bounds__(kRunBlock) void k_quotes_fill(QuotesArgs a) {
  const uint64_t j = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (j >= a.n_script) return;
  const uint32_t r = a.words[j].region;
  if (r == FS_NONE) return;
  if (j == 0 || a.words[j - 1].region == FS_NONE) a.regions[r].first = (uint32_t)j;
  if (j + 1 == a.n_script || a.words[j + 1].region == FS_NONE) a.regions[r].last = (uint32_t)j;
}

struct RegionAcc {
  uint32_t n_words, n_exact, peak, peak_first, peak_last;
};

// one lane per region; a region of kLong words or more by the whole wave
__global__ __launch_bounds__(kRunBlock) void k_quotes_reduce(QuotesArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const bool live = r < a.n_regions;
  uint32_t first = 0, last = 0;
  if (live) {
    first = a.regions[r].first;
    last = a.regions[r].last;
  }
  const bool is_long = live && last - first + 1 >= kLong;
  RegionAcc acc{0, 0, 0, 0, 0};
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)first, j);
    const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)last, j);
    uint32_t nw = 0, nx = 0, pk = 0, pf = FS_NONE;
    for (uint64_t w = (uint64_t)fj + lane; w <= lj; w += kWave) {
      const fs_quote_word q = a.words[w];
      nw += q.n_words;
      nx += q.n_exact;
      if (q.n_passage_works > pk) {                  // (ascending w: the first one at the peak)
        pk = q.n_passage_works;
        pf = (uint32_t)w;
      }
    }
    nw = wave_sum(nw);
    nx = wave_sum(nx);
    for (uint32_t d = 32; d; d >>= 1) {
      const uint32_t ok = __shfl_xor(pk, d), of = __shfl_xor(pf, d);
      if (ok > pk || (ok == pk && of < pf)) {
        pk = ok;
        pf = of;
      }
    }
    // the run at the peak that starts there: up to the first word behind it that differs
    uint32_t pl = lj;
    for (uint64_t c = (uint64_t)pf + 1; c <= lj; c += kWave) {
      const uint64_t w = c + lane;
      const uint64_t m = __ballot(w <= lj && a.words[w].n_passage_works != pk);
      if (m) {
        pl = (uint32_t)(c + (uint32_t)__builtin_ctzll(m)) - 1;
        break;
      }
    }
    if ((int)lane == j) acc = RegionAcc{nw, nx, pk, pf, pl};
  }
  if (live && !is_long) {
    bool open = false;
    for (uint32_t w = first; w <= last; ++w) {
      const fs_quote_word q = a.words[w];
      acc.n_words += q.n_words;
      acc.n_exact += q.n_exact;
      const uint32_t v = q.n_passage_works;
      if (v > acc.peak) {
        acc.peak = v;
        acc.peak_first = acc.peak_last = w;
        open = true;
      } else if (v == acc.peak && open) {
        acc.peak_last = w;
      } else {
        open = false;
      }
    }
  }
  if (live) {
    fs_quote_region o{};
    o.first = first;
    o.last = last;
    // spans that start at or before `last`, less those that end before `first`
    o.n_passages = a.s0[last] - a.s0[first] + a.words[first].n_passages;
    o.n_works = 0;                                   // k_quotes_slices<1>, k_quotes_each<1>
    o.n_words = acc.n_words;
    o.n_exact = acc.n_exact;
    o.peak = acc.peak;
    o.peak_first = acc.peak_first;
    o.peak_last = acc.peak_last;
    a.regions[r] = o;
  }
}

// device scratch of one call
struct QuotesScratch {
  DBuf<uint32_t> wstart, wend, diff, starts, s0, hc, area, rarea, status;
  fs_runs* runs = nullptr;
  ~QuotesScratch() { if (runs) fs_runs_free(runs); }
};

// the rules both entry points share; *done when no record is left to look at
int quotes_check(uint64_t n_rows, uint32_t n_script, uint32_t min_words, uint32_t min_works,
                 const void* words, const void* regions, uint64_t cap, uint64_t* n_regions,
                 bool* done) {
  *done = false;
  if (!n_regions || (n_script && !words) || (cap && !regions)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_works == 0) {
    fs_set_error("min_words and min_works must be at least 1");
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("quotes", n_rows, n_script));
  *n_regions = 0;
  *done = n_rows == 0;
  return FS_OK;
}

int quotes_invalid() {
  fs_set_error("a work >= n_works or an orig_ix >= n_script");
  return FS_E_INVALID;
}

template <class K>
int lds_allow(K kernel, size_t lds) {
  if (lds > kLdsMax) {
    fs_set_error("%zu bytes of LDS", lds);
    return FS_E_UNSUPPORTED;
  }
  if (lds > 64 * 1024)
    FS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return FS_OK;
}

// d_words written and *n_regions set; d_regions too unless FS_E_CAPACITY (all on `s`, finished
// on return).
int quotes_run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
               uint32_t min_words, uint32_t max_gap, uint32_t min_works, fs_quote_word* d_words,
               fs_quote_region* d_regions, uint64_t cap, uint64_t* n_regions, hipStream_t s) {
  const RowsSrc src{d_rows};
  if (!n) {
    if (n_script)
      hipLaunchKernelGGL(k_quotes_none, dim3((n_script + kRunBlock - 1) / kRunBlock),
                         dim3(kRunBlock), 0, s, d_words, n_script);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }
  QuotesScratch k;
  QuotesArgs a{};
  a.n = n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.bw = (n_script + 31) / 32;
  a.min_words = min_words;
  a.min_works = min_works;
  a.slice = kSlice;
  // a wave per work until the waves outnumber what the GPU holds at once several times over
  a.per_wave = n_works >= (1u << 18) ? kWorksPerWave : 1;
  // a slice is at least as many records as its merge areas have words (two bits per script
  // word, and a bit per region: a region takes two words of the script at least): merging
  // never costs more than reducing, and the areas stay below four bytes per record
  while (a.slice < 2 * (size_t)a.bw + a.bw / 2 + 1) a.slice *= 2;
  const uint32_t tiles = (uint32_t)(((uint64_t)n + a.slice - 1) / a.slice);

  FS_TRY(fs_runs_find(d_rows, n, min_words, max_gap, s, &k.runs, &a.heads, &a.n_runs));
  if (!n_works || !n_script) return quotes_invalid();

  FS_TRY(k.wstart.reserve(n_works));
  FS_TRY(k.wend.reserve(n_works));
  FS_TRY(k.diff.reserve((size_t)n_script + 1));
  FS_TRY(k.starts.reserve(n_script));
  FS_TRY(k.s0.reserve(n_script));
  FS_TRY(k.hc.reserve(n_script));
  FS_TRY(k.status.reserve(4));
  FS_TRY(k.area.reserve((size_t)tiles * 2 * a.bw));
  FS_HIP(hipMemsetAsync(k.wstart.p, 0, (size_t)n_works * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.wend.p, 0, (size_t)n_works * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.diff.p, 0, ((size_t)n_script + 1) * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.starts.p, 0, (size_t)n_script * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.status.p, 0, 4 * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.area.p, 0, (size_t)tiles * 2 * a.bw * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(d_words, 0, (size_t)n_script * sizeof(fs_quote_word), s));
  a.wstart = k.wstart.p;
  a.wend = k.wend.p;
  a.diff = k.diff.p;
  a.starts = k.starts.p;
  a.s0 = k.s0.p;
  a.hc = k.hc.p;
  a.area = k.area.p;
  a.status = k.status.p;
  a.words = d_words;
  a.regions = d_regions;

  const size_t lds_slices = (size_t)a.bw * sizeof(uint32_t), lds_each = 2 * lds_slices;
  FS_TRY(lds_allow(&k_quotes_slices<0>, lds_slices));
  FS_TRY(lds_allow(&k_quotes_each<0>, lds_each));
  const uint32_t each_blocks = (n_works + a.per_wave - 1) / a.per_wave;
  hipLaunchKernelGGL(k_quotes_runs, dim3((a.n_runs + kRunBlock - 1) / kRunBlock),
                     dim3(kRunBlock), 0, s, src, a);
  hipLaunchKernelGGL((k_quotes_slices<0>), dim3(tiles), dim3(kWave), lds_slices, s, src, a);
  hipLaunchKernelGGL((k_quotes_each<0>), dim3(each_blocks), dim3(kWave), lds_each, s, src, a);
  hipLaunchKernelGGL(k_quotes_scan, dim3(1), dim3(kScanBlock), 0, s, a);
  FS_HIP(hipGetLastError());
  uint32_t st[2];
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[0]) return quotes_invalid();
  *n_regions = st[1];
  if (st[1] > cap) return FS_E_CAPACITY;
  if (!st[1]) return FS_OK;

  a.n_regions = st[1];
  a.rbw = (a.n_regions + 31) / 32;
  FS_TRY(k.rarea.reserve((size_t)tiles * a.rbw));
  FS_HIP(hipMemsetAsync(k.rarea.p, 0, (size_t)tiles * a.rbw * sizeof(uint32_t), s));
  a.rarea = k.rarea.p;
  const size_t lds_regions = (size_t)a.rbw * sizeof(uint32_t);
  FS_TRY(lds_allow(&k_quotes_each<1>, lds_regions));
  hipLaunchKernelGGL(k_quotes_fill, dim3((n_script + kRunBlock - 1) / kRunBlock), dim3(kRunBlock),
                     0, s, a);
  hipLaunchKernelGGL(k_quotes_reduce, dim3((a.n_regions + kRunBlock - 1) / kRunBlock),
                     dim3(kRunBlock), 0, s, a);
  hipLaunchKernelGGL((k_quotes_slices<1>), dim3(tiles), dim3(kWave), 0, s, src, a);
  hipLaunchKernelGGL((k_quotes_each<1>), dim3(each_blocks), dim3(kWave), lds_regions, s, src,
                     a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

}  // namespace

extern "C" int fs_quotes(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, const double* comb, uint64_t n_rows,
                         uint32_t n_works, uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                         uint32_t min_works, fs_quote_word* words, fs_quote_region* regions,
                         uint64_t cap, uint64_t* n_regions) {
  bool done = false;
  FS_TRY(quotes_check(n_rows, n_script, min_words, min_works, words, regions, cap, n_regions,
                      &done));
  if (done) {
    fs_quote_word w{};
    w.region = FS_NONE;
    for (uint32_t j = 0; j < n_script; ++j) words[j] = w;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix || !comb) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  // regions never outnumber half the script's words (a word apart at least) nor the records
  uint64_t most = ((uint64_t)n_script + 1) / 2;
  if (most > n_rows) most = n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_quote_word> d_words;
  DBuf<fs_quote_region> d_regions;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n, nullptr, comb));
  FS_TRY(d_words.reserve(n_script));
  FS_TRY(d_regions.reserve(cap < most ? cap : most));
  const int rc = quotes_run(rows.p, n, n_works, n_script, min_words, max_gap, min_works, d_words.p,
                            d_regions.p, cap, n_regions, nullptr);
  if (rc != FS_OK && rc != FS_E_CAPACITY) return rc;
  FS_TRY(copy_out(words, d_words, n_script));
  if (rc == FS_OK && *n_regions) FS_TRY(copy_out(regions, d_regions, *n_regions));
  FS_HIP(hipDeviceSynchronize());
  return rc;
}

extern "C" int fs_quotes_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                              uint32_t min_words, uint32_t max_gap, uint32_t min_works,
                              fs_quote_word* d_words, fs_quote_region* d_regions, uint64_t cap,
                              uint64_t* n_regions) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: quotes take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  bool done = false;
  FS_TRY(quotes_check(n_rows, (uint32_t)ix->n_script, min_words, min_works, d_words, d_regions,
                      cap, n_regions, &done));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_words & 3) ||
      ((uintptr_t)d_regions & 3)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_words and d_regions 4-byte");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  return quotes_run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                    min_works, d_words, d_regions, cap, n_regions, ix->stream);
}
