// fs_works.hip -- `ao3.py works`: match records sorted by (work, fan_ix) reduced by work
// (fs_works, fs_works_rows in include/fandom_search.h): per work its extent, distinct script
// words, passage statistics, threshold counts and record counts per group (scene or
// character), plus the non-zero (work, group) cells in order.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   fs_runs_find    the run heads of fs_passages.hip (and its sortedness check)
//   k_works_runs    one lane per run: work boundaries (every work starts a run), the work's
//                   passage statistics by atomics, one set per wave where a wave holds one work
//   k_works_scan    one workgroup: where each work's cells go in the staging list
//   k_works_slices  works of more than `slice` records: a wave per slice of records reduces its
//                   part in LDS and merges it into the work's global bitmap and counters
//   k_works_each    a wave per work (per kWorksPerWave works when they are many): a work of at most `slice` records reduced
//                   in LDS (bit per script word, two counters per group), a larger one read
//                   back from its global area; summary, counts and staged cells written
//   k_works_scan    again, over the works' cell counts
//   k_works_cells   staged cells to their final places: sorted by (work, group), no sort
// A workgroup is one wave with its own LDS: the bitmap and counters sized from n_script and
// n_groups, so the usual 5 KB runs 32 waves per CU and only the limit case (96 KB) one.
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kSlice = 8192;          // records per slice of a large work, at least (works_run)
constexpr uint32_t kWorksPerWave = 8;       // works a wave takes when there are many (works_run)
constexpr uint32_t kDepth = 4;              // chunks of 64 records whose loads are in flight together
constexpr uint32_t kScanItems = 4;          // works per thread of the one-workgroup scan
constexpr uint32_t kRunBlock = 256;

struct WorksArgs {
  uint32_t n, n_works, n_script, bw, n_groups, n_thr, slice, min_words, per_wave;
  const uint32_t* group_of;     // [n_script] or nullptr (n_groups == 0)
  const double* thr;            // [n_thr]
  uint32_t* wstart;             // [n_works] first record of a work
  uint32_t* wend;               // [n_works] one past its last (both 0: no records)
  uint32_t* pstats;             // [n_works][3] passages, records in them, longest
  uint32_t* toff;               // [n_works] staging position of a work's cells
  uint32_t* coff;               // [n_works] final position
  uint32_t* area;               // [tiles][bw + 2 * n_groups] merge areas of large works
  uint32_t* status;             // [0] invalid input, [1] staged cells, [2] cells
  fs_work* out;
  uint32_t* counts;             // [n_works][n_thr + 1], zeroed before the kernels
  fs_work_cell* staged;
  fs_work_cell* cells;
};

// one lane per run
__global__ __launch_bounds__(kRunBlock) void k_works_runs(RowsSrc src, WorksArgs a,
                                                          const uint32_t* __restrict__ heads,
                                                          uint32_t n_runs) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  bool keep = false, bad = false;
  uint32_t w = 0, len = 0;
  if (r < n_runs) {
    const uint32_t h = heads[r];
    len = heads[r + 1] - h;
    w = src.key(h).x;
    if (w >= a.n_works) {
      bad = true;
    } else {
      const uint32_t pw = h ? src.key(h - 1).x : FS_NONE;
      if (pw != w) {
        a.wstart[w] = h;
        if (h && pw < a.n_works) a.wend[pw] = h;
      }
      if (r + 1 == n_runs) a.wend[w] = a.n;
      keep = len >= a.min_words;
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
  const uint64_t mk = __ballot(keep);
  if (!mk) return;
  const int first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(mk));
  const uint32_t wf = (uint32_t)__builtin_amdgcn_readlane((int)w, first);
  if (__ballot(keep && w == wf) == mk) {            // one work in this wave: one set of atomics
    const uint32_t sum = wave_sum(keep ? len : 0u), top = wave_max(keep ? len : 0u);
    if ((int)lane == first) {
      atomicAdd(&a.pstats[3 * (size_t)wf], (uint32_t)__popcll(mk));
      atomicAdd(&a.pstats[3 * (size_t)wf + 1], sum);
      atomicMax(&a.pstats[3 * (size_t)wf + 2], top);
    }
  } else if (keep) {
    atomicAdd(&a.pstats[3 * (size_t)w], 1u);
    atomicAdd(&a.pstats[3 * (size_t)w + 1], len);
    atomicMax(&a.pstats[3 * (size_t)w + 2], len);
  }
}

// exclusive scan over the works (one workgroup, chunks of 4096 in turn) of
//   kind 0: the most cells a work can have, min(records, groups) -> toff, status[1]
//   kind 1: the cells it has -> coff, status[2]
template <int kKind>
__global__ __launch_bounds__(kScanBlock) void k_works_scan(WorksArgs a) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  uint32_t* __restrict__ dst = kKind ? a.coff : a.toff;
  const uint32_t cells = scan_chunks<kScanItems, uint32_t, uint32_t>(
      a.n_works,
      [&a](uint64_t j) -> uint32_t {
        if (kKind) return a.out[j].n_groups_hit;
        const uint32_t nw = a.wend[j] - a.wstart[j];
        return nw < a.n_groups ? nw : a.n_groups;
      },
      [dst](uint64_t j, uint32_t at, uint32_t) { dst[j] = at; }, s_w);
  if (threadIdx.x == 0) a.status[kKind ? 2 : 1] = cells;
}

// A wave's LDS: bit per script word, then records and exact records per group.
struct Lds {
  uint32_t* bm;
  uint32_t* cnt;
  uint32_t* cntx;
};

__device__ inline Lds lds_of(uint32_t* mem, const WorksArgs& a) {
  return Lds{mem, mem + a.bw, mem + a.bw + a.n_groups};
}

__device__ inline void lds_clear(uint32_t* mem, const WorksArgs& a) {
  for (uint32_t k = threadIdx.x; k < a.bw + 2 * a.n_groups; k += kWave) mem[k] = 0;
}

// Records [b, e) (wave-uniform) into the wave's LDS.  Returns this lane's share of the
// outputs: lane j < n_thr the records with comb <= thr[j]; *fresh += script words whose bit
// these records set first (wave-uniform); *bad |= an orig_ix outside the script.
__device__ inline uint32_t lds_add(const RowsSrc& src, const WorksArgs& a, const Lds& l, uint64_t b,
                                   uint64_t e, uint32_t* fresh, bool* bad) {
  const uint32_t lane = threadIdx.x;
  uint32_t acc = 0;
  for (uint64_t c = b; c < e; c += kDepth * kWave) {
    uint32_t os[kDepth];
    double vs[kDepth];
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {           // the loads of kDepth chunks in flight
      const uint64_t i = c + u * kWave + lane;
      os[u] = i < e ? src.key(i).z : 0u;
      vs[u] = i < e ? src.comb(i) : __builtin_nan("");
    }
#pragma unroll
    for (uint32_t u = 0; u < kDepth; ++u) {
      const uint64_t i = c + u * kWave + lane;
      if (c + u * kWave >= e) break;                  // (wave-uniform)
      const uint32_t o = os[u];
      const double v = vs[u];
      bool first = false;
      if (i < e) {
        if (o < a.n_script) {
          const uint32_t bit = 1u << (o & 31);
          first = !(atomicOr(&l.bm[o >> 5], bit) & bit);
          if (a.n_groups) {
            const uint32_t g = a.group_of[o];        // < n_groups: checked on the host
            atomicAdd(&l.cnt[g], 1u);
            if (v <= 0.0) atomicAdd(&l.cntx[g], 1u);
          }
        } else {
          *bad = true;
        }
      }
      *fresh += (uint32_t)__popcll(__ballot(first));
      for (uint32_t j = 0; j < a.n_thr; ++j) {
        const uint32_t k = (uint32_t)__popcll(__ballot(i < e && v <= a.thr[j]));
        if (lane == j) acc += k;
      }
    }
  }
  return acc;
}

// the bits records [b, e) set, cleared again: all of them when that is less work
__device__ inline void lds_unset(const RowsSrc& src, const WorksArgs& a, const Lds& l, uint64_t b,
                                 uint64_t e) {
  if (e - b >= a.bw) {
    for (uint32_t k = threadIdx.x; k < a.bw; k += kWave) l.bm[k] = 0;
    return;
  }
  for (uint64_t i = b + threadIdx.x; i < e; i += kWave) {
    const uint32_t o = src.key(i).z;
    if (o < a.n_script) l.bm[o >> 5] = 0;
  }
}

extern __shared__ uint32_t s_works[];

// a wave per slice of records: the parts of large works inside it
__global__ __launch_bounds__(kWave) void k_works_slices(RowsSrc src, WorksArgs a) {
  const Lds l = lds_of(s_works, a);
  const uint32_t lane = threadIdx.x;
  lds_clear(s_works, a);
  __syncthreads();
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
    uint32_t fresh = 0;
    const uint32_t acc = lds_add(src, a, l, b, e, &fresh, &bad);
    __syncthreads();
    uint32_t* __restrict__ g = a.area + (size_t)(ws / a.slice) * (a.bw + 2 * a.n_groups);
    for (uint32_t k = lane; k < a.bw; k += kWave) {
      const uint32_t v = l.bm[k];
      if (v) {
        atomicOr(&g[k], v);
        l.bm[k] = 0;
      }
    }
    for (uint32_t k = lane; k < 2 * a.n_groups; k += kWave) {
      const uint32_t v = l.cnt[k];                  // cnt and cntx are one array
      if (v) {
        atomicAdd(&g[a.bw + k], v);
        l.cnt[k] = 0;
      }
    }
    if (lane < a.n_thr && acc) atomicAdd(&a.counts[(size_t)w * (a.n_thr + 1) + lane], acc);
    __syncthreads();
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
}

// a wave per a.per_wave works
__global__ __launch_bounds__(kWave) void k_works_each(RowsSrc src, WorksArgs a) {
  const Lds l = lds_of(s_works, a);
  const uint32_t lane = threadIdx.x;
  lds_clear(s_works, a);
  __syncthreads();
  const uint64_t w0 = (uint64_t)blockIdx.x * a.per_wave;
  const uint64_t w1 = w0 + a.per_wave < a.n_works ? w0 + a.per_wave : a.n_works;
  bool bad = false;
  for (uint64_t w = w0; w < w1; ++w) {
    const uint32_t ws = a.wstart[w], we = a.wend[w], nw = we - ws;
    fs_work o{};
    o.top_group = FS_NONE;
    if (nw == 0) {
      if (lane == 0) a.out[w] = o;
      continue;
    }
    uint32_t distinct = 0;
    const bool large = nw > a.slice;
    if (!large) {
      const uint32_t acc = lds_add(src, a, l, ws, we, &distinct, &bad);
      if (lane < a.n_thr) a.counts[w * (a.n_thr + 1) + lane] = acc;
      __syncthreads();
      lds_unset(src, a, l, ws, we);
    } else {
      const uint32_t* __restrict__ g = a.area + (size_t)(ws / a.slice) * (a.bw + 2 * a.n_groups);
      for (uint32_t k = lane; k < a.bw; k += kWave) distinct += (uint32_t)__popc(g[k]);
      distinct = wave_sum(distinct);
      for (uint32_t k = lane; k < 2 * a.n_groups; k += kWave) l.cnt[k] = g[a.bw + k];
      __syncthreads();
    }
    // the groups in order: cells staged, counters cleared, the first largest one kept
    uint32_t hit = 0, best = 0, best_g = FS_NONE;
    const uint32_t tpos = a.toff[w];
    for (uint32_t g0 = 0; g0 < a.n_groups; g0 += kWave) {
      const uint32_t g = g0 + lane;
      uint32_t c = 0, x = 0;
      if (g < a.n_groups) {
        c = l.cnt[g];
        x = l.cntx[g];
        if (c) {
          l.cnt[g] = 0;
          l.cntx[g] = 0;
        }
      }
      const uint64_t m = __ballot(c != 0);
      if (c) {
        fs_work_cell cell;
        cell.work = (uint32_t)w;
        cell.group = g;
        cell.n_words = c;
        cell.n_exact = x;
        a.staged[(size_t)tpos + hit + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = cell;
      }
      hit += (uint32_t)__popcll(m);
      const uint32_t mx = wave_max(c);
      if (mx > best) {
        best = mx;
        best_g = g0 + (uint32_t)__builtin_ctzll(__ballot(c == mx));
      }
    }
    __syncthreads();
    if (lane == 0) {
      o.first = ws;
      o.n_words = nw;
      o.fan_first = src.key(ws).y;
      o.fan_last = src.key((uint64_t)we - 1).y;
      o.n_script_words = distinct;
      o.n_passages = a.pstats[3 * w];
      o.passage_words = a.pstats[3 * w + 1];
      o.longest = a.pstats[3 * w + 2];
      o.n_groups_hit = hit;
      o.top_group = best_g;
      o.top_group_words = best;
      a.out[w] = o;
      a.counts[w * (a.n_thr + 1) + a.n_thr] = nw;
    }
  }
  if (__ballot(bad) && lane == 0) atomicOr(&a.status[0], 1u);
}

// staged cells to their places: a lane per work where the wave's works have few cells, else
// the wave takes its works in turn
__global__ __launch_bounds__(kRunBlock) void k_works_cells(WorksArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  uint32_t cnt = 0, from = 0, to = 0;
  if (w < a.n_works) {
    cnt = a.out[w].n_groups_hit;
    from = a.toff[w];
    to = a.coff[w];
  }
  const uint32_t most = wave_max(cnt);
  if (most <= 4) {
    for (uint32_t k = 0; k < cnt; ++k) a.cells[(size_t)to + k] = a.staged[(size_t)from + k];
    return;
  }
  for (uint64_t m = __ballot(cnt != 0); m; m &= m - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
    const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)cnt, j);
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)from, j);
    const uint32_t tj = (uint32_t)__builtin_amdgcn_readlane((int)to, j);
    for (uint32_t k = lane; k < cj; k += kWave) a.cells[(size_t)tj + k] = a.staged[(size_t)fj + k];
  }
}

// device scratch of one call
struct WorksScratch {
  DBuf<uint32_t> wstart, wend, pstats, toff, coff, area, status, group_of;
  DBuf<double> thr;
  DBuf<fs_work_cell> staged;
  fs_runs* runs = nullptr;
  ~WorksScratch() { if (runs) fs_runs_free(runs); }
};

// the rules both entry points share; *done when no record is left to look at
int works_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint32_t* group_of,
                uint32_t n_groups, uint32_t min_words, const double* thresholds, uint32_t n_thr,
                const void* out, const void* counts, const void* cells, uint64_t cap,
                uint64_t* n_cells, bool* done) {
  *done = false;
  if (!n_cells || !thresholds || (n_works && (!out || !counts)) || (cap && !cells) ||
      (n_groups && !group_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (!n_thr || n_thr > 64) {
    fs_set_error("n_thr outside 1..64");
    return FS_E_INVALID;
  }
  for (uint32_t t = 1; t < n_thr; ++t)
    if (!(thresholds[t - 1] <= thresholds[t])) {
      fs_set_error("thresholds must ascend");
      return FS_E_INVALID;
    }
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: works take fewer than 2^32", (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  if (n_script > FS_WORKS_MAX_SCRIPT || n_groups > FS_WORKS_MAX_GROUPS) {
    fs_set_error("n_script %u, n_groups %u: works take up to %u and %u", n_script, n_groups,
                 FS_WORKS_MAX_SCRIPT, FS_WORKS_MAX_GROUPS);
    return FS_E_UNSUPPORTED;
  }
  for (uint32_t i = 0; n_groups && i < n_script; ++i)
    if (group_of[i] >= n_groups) {
      fs_set_error("group_of[%u] = %u with %u groups", i, group_of[i], n_groups);
      return FS_E_INVALID;
    }
  *n_cells = 0;
  *done = n_rows == 0;
  return FS_OK;
}

int works_invalid() {
  fs_set_error("a work >= n_works or an orig_ix >= n_script");
  return FS_E_INVALID;
}

// d_out and d_counts written and *n_cells set; d_cells too unless FS_E_CAPACITY (all on `s`,
// finished on return).
int works_run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
              const uint32_t* group_of, uint32_t n_groups, uint32_t min_words, uint32_t max_gap,
              const double* thresholds, uint32_t n_thr, fs_work* d_out, uint32_t* d_counts,
              fs_work_cell* d_cells, uint64_t cap, uint64_t* n_cells, hipStream_t s) {
  const RowsSrc src{d_rows};
  WorksScratch k;
  WorksArgs a{};
  a.n = n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.bw = n_script ? (n_script + 31) / 32 : 1;
  a.n_groups = n_groups;
  a.n_thr = n_thr;
  a.min_words = min_words;
  a.slice = kSlice;
  // a wave per work until the waves outnumber what the GPU holds at once several times over
  a.per_wave = n_works >= (1u << 18) ? kWorksPerWave : 1;
  const size_t per_area = (size_t)a.bw + 2 * (size_t)n_groups;
  // a slice is at least as many records as its merge area has words: merging never costs more
  // than reducing, and the areas stay below four bytes per record
  while (a.slice < per_area) a.slice *= 2;
  const uint32_t tiles = n ? (uint32_t)(((uint64_t)n + a.slice - 1) / a.slice) : 0;
  const size_t lds = per_area * sizeof(uint32_t);

  const uint32_t* heads = nullptr;
  uint32_t n_runs = 0;
  if (n) FS_TRY(fs_runs_find(d_rows, n, min_words, max_gap, s, &k.runs, &heads, &n_runs));
  if (n && !n_works) return works_invalid();
  if (!n_works) return FS_OK;

  FS_TRY(k.wstart.reserve(n_works));
  FS_TRY(k.wend.reserve(n_works));
  FS_TRY(k.pstats.reserve(3 * (size_t)n_works));
  FS_TRY(k.toff.reserve(n_works));
  FS_TRY(k.coff.reserve(n_works));
  FS_TRY(k.status.reserve(4));
  FS_TRY(k.area.reserve((size_t)tiles * per_area));
  FS_TRY(k.thr.upload(thresholds, n_thr, s));
  if (n_groups) FS_TRY(k.group_of.upload(group_of, n_script, s));
  FS_HIP(hipMemsetAsync(k.wstart.p, 0, (size_t)n_works * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.wend.p, 0, (size_t)n_works * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.pstats.p, 0, 3 * (size_t)n_works * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(k.status.p, 0, 4 * sizeof(uint32_t), s));
  if (tiles) FS_HIP(hipMemsetAsync(k.area.p, 0, (size_t)tiles * per_area * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_works * (n_thr + 1) * sizeof(uint32_t), s));
  a.group_of = n_groups ? k.group_of.p : nullptr;
  a.thr = k.thr.p;
  a.wstart = k.wstart.p;
  a.wend = k.wend.p;
  a.pstats = k.pstats.p;
  a.toff = k.toff.p;
  a.coff = k.coff.p;
  a.area = k.area.p;
  a.status = k.status.p;
  a.out = d_out;
  a.counts = d_counts;
  a.cells = d_cells;

  if (n_runs)
    hipLaunchKernelGGL(k_works_runs, dim3((n_runs + kRunBlock - 1) / kRunBlock),
                       dim3(kRunBlock), 0, s, src, a, heads, n_runs);
  hipLaunchKernelGGL(k_works_scan<0>, dim3(1), dim3(kScanBlock), 0, s, a);
  FS_HIP(hipGetLastError());
  uint32_t st[3];
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[0]) return works_invalid();
  FS_TRY(k.staged.reserve(st[1]));
  a.staged = k.staged.p;

  if (lds > 64 * 1024) {
    FS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_works_slices),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_works_each),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  if (tiles) hipLaunchKernelGGL(k_works_slices, dim3(tiles), dim3(kWave), lds, s, src, a);
  hipLaunchKernelGGL(k_works_each, dim3((n_works + a.per_wave - 1) / a.per_wave),
                     dim3(kWave), lds, s, src, a);
  hipLaunchKernelGGL(k_works_scan<1>, dim3(1), dim3(kScanBlock), 0, s, a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[0]) return works_invalid();
  *n_cells = st[2];
  if (st[2] > cap) return FS_E_CAPACITY;
  if (st[2]) {
    hipLaunchKernelGGL(k_works_cells, dim3((n_works + kRunBlock - 1) / kRunBlock), dim3(kRunBlock),
                       0, s, a);
    FS_HIP(hipGetLastError());
  }
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

}  // namespace

extern "C" int fs_works(int device, const uint32_t* work, const uint32_t* fan_ix,
                        const uint32_t* orig_ix, const double* comb, uint64_t n_rows,
                        uint32_t n_works, uint32_t n_script, const uint32_t* group_of,
                        uint32_t n_groups, uint32_t min_words, uint32_t max_gap,
                        const double* thresholds, uint32_t n_thr, fs_work* out, uint32_t* counts,
                        fs_work_cell* cells, uint64_t cap, uint64_t* n_cells) {
  bool done = false;
  FS_TRY(works_check(n_rows, n_works, n_script, group_of, n_groups, min_words, thresholds, n_thr,
                     out, counts, cells, cap, n_cells, &done));
  if (done) {
    fs_work o{};
    o.top_group = FS_NONE;
    for (uint32_t w = 0; w < n_works; ++w) out[w] = o;
    for (size_t k = 0; k < (size_t)n_works * (n_thr + 1); ++k) counts[k] = 0;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix || !comb) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_counts;
  DBuf<fs_work> d_out;
  DBuf<fs_work_cell> d_cells;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n, nullptr, comb));
  FS_TRY(d_out.reserve(n_works));
  FS_TRY(d_counts.reserve((size_t)n_works * (n_thr + 1)));
  FS_TRY(d_cells.reserve(cap < n_rows ? cap : n_rows));       // a record makes at most one cell
  const int rc = works_run(rows.p, n, n_works, n_script, group_of, n_groups, min_words, max_gap,
                           thresholds, n_thr, d_out.p, d_counts.p, d_cells.p, cap, n_cells,
                           nullptr);
  if (rc != FS_OK && rc != FS_E_CAPACITY) return rc;
  if (n_works) {
    FS_TRY(copy_out(out, d_out, n_works));
    FS_TRY(copy_out(counts, d_counts, (size_t)n_works * (n_thr + 1)));
  }
  if (rc == FS_OK && *n_cells) FS_TRY(copy_out(cells, d_cells, *n_cells));
  FS_HIP(hipDeviceSynchronize());
  return rc;
}

extern "C" int fs_works_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                             const uint32_t* group_of, uint32_t n_groups, uint32_t min_words,
                             uint32_t max_gap, const double* thresholds, uint32_t n_thr,
                             fs_work* d_out, uint32_t* d_counts, fs_work_cell* d_cells,
                             uint64_t cap, uint64_t* n_cells) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: works take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  bool done = false;
  FS_TRY(works_check(n_rows, n_works, (uint32_t)ix->n_script, group_of, n_groups, min_words,
                     thresholds, n_thr, d_out, d_counts, d_cells, cap, n_cells, &done));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_out & 7) ||
      ((uintptr_t)d_cells & 15) || ((uintptr_t)d_counts & 3)) {
    fs_set_error("d_rows and d_cells must be 16-byte aligned device pointers, d_out 8-byte");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  return works_run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, group_of, n_groups,
                   min_words, max_gap, thresholds, n_thr, d_out, d_counts, d_cells, cap, n_cells,
                   ix->stream);
}
