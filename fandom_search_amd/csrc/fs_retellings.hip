// fs_retellings.hip -- `ao3.py retellings`: works that quote the script in its order
// (fs_retellings, fs_retellings_rows in include/fandom_search.h).  The passages of fs_passages,
// numbered in record order; inside a work passage i may follow an earlier passage j when
// orig_first(i) > orig_last(j), and the work's chain is the heaviest sequence of passages each
// following the one before:
//   best(i) = n_words(i) + max(0, max over such j of best(j)), prev(i) the smallest j at the
//   maximum, the chain's end the smallest i with the largest best.
// Candidates are compared as one 64-bit key, best in the high half and ~j in the low half, so
// that a plain maximum gives both tie rules and the order in which candidates are looked at
// does not matter: every output is an integer and no schedule changes it.
//
// Separate launches; no workgroup waits on another:
//   k_rt_check      one lane per record: work < n_works
//   (fs_runs_find)  the run heads, as fs_passages joins them
//   k_rt_kept       one lane per run: kept runs counted per workgroup, then (after k_rt_scan)
//                   placed in record order with their seven plain fields
//   k_rt_offsets    one lane per work: its first passage (the passages are sorted by work)
//   k_rt_bin        one lane per work: its class by passage count, counted per workgroup, then
//                   (after k_rt_scan) listed
//   k_rt_chain_small  a lane per work of up to FS_RETELLINGS_SMALL passages
//   k_rt_chain_wave   a wave per larger work, i in tiles of 64: every lane first takes its
//                   maximum over all earlier tiles (64 candidates per load, handed round by
//                   readlane), then the tile is resolved in 64 cross-lane steps.  Works of up to
//                   FS_RETELLINGS_LDS passages keep {orig_last, best, depth} in LDS, longer ones
//                   read them back from global memory.
//   k_rt_trace      one lane per work: prev walked back from the end, chain_pos = depth, the
//                   per-work record
//   k_rt_write      one lane per passage: the passage records
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSmallDefault = 8;
constexpr uint32_t kLdsDefault = 4096;
constexpr uint32_t kLdsMax = 4096;             // 12 bytes a passage: 48 KiB of LDS a wave

static_assert(sizeof(fs_retelling) == 40 && sizeof(fs_retelling_passage) == 48, "fs_retellings");

// status words
enum { kStBad = 0, kStTotal = 1, kStMedium = 2, kStLarge = 3, kStMaxMedium = 4, kStWords = 8 };

struct RtArgs {
  const uint32_t* heads;         // [n_runs + 1]
  uint32_t n, n_runs, n_works, min_words, n_pass;
  uint32_t small, lds;           // the largest passage counts of the small and of the LDS class
  uint32_t work_blocks;
  uint32_t* cnt;                 // [workgroups of runs] kept runs, then their exclusive scan
  uint32_t* first;               // [n_pass] each: the plain fields ...
  uint32_t* nw;
  uint32_t* work;
  uint32_t* ff;
  uint32_t* fl;
  uint32_t* of;
  uint32_t* ol;
  uint32_t* best;                //          ... and the chain's
  uint32_t* prev;
  uint32_t* depth;
  uint32_t* cpos;
  uint32_t* woff;                // [n_works + 1] passages in front of the work's
  uint32_t* wend;                // [n_works] the chain's end, descents, words in passages
  uint32_t* wdesc;
  uint32_t* wwords;
  uint32_t* bcnt;                // [2 * work_blocks] medium, then large works per workgroup
  uint32_t* list;                // [n_works] the medium works, then the large ones
  uint32_t* status;
  fs_retelling* out;
  fs_retelling_passage* passages;
};

__global__ __launch_bounds__(kBlock) void k_rt_check(RowsSrc src, RtArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool bad = i < a.n && src.key(i).x >= a.n_works;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStBad], 1u);
}

// exclusive scan of in[0..nb) into out (which may be in), *total = sum (one workgroup, chunks
// of 1024 in turn)
__global__ __launch_bounds__(kScanBlock) void k_rt_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t nb, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, nb, out, total);
}

// kPlace false: kept runs of this workgroup's 256 runs into cnt; true: the kept runs to their
// places, cnt holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_rt_kept(RowsSrc src, RtArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  uint32_t b = 0, e = 0;
  if (r < a.n_runs) {
    b = a.heads[r];
    e = a.heads[r + 1];
  }
  const bool keep = r < a.n_runs && e - b >= a.min_words;
  uint32_t rank, total;
  block_rank<kBlock>(keep, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = total;
  } else if (keep) {
    const uint32_t p = a.cnt[blockIdx.x] + rank;
    const uint4 x = src.key(b), y = src.key(e - 1);
    a.first[p] = b;
    a.nw[p] = e - b;
    a.work[p] = x.x;
    a.ff[p] = x.y;
    a.fl[p] = y.y;
    a.of[p] = x.z;
    a.ol[p] = y.z;
  }
}

// woff[w] = the passages of works below w (work[] ascends); woff[n_works] = n_pass
__global__ __launch_bounds__(kBlock) void k_rt_offsets(RtArgs a) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w > a.n_works) return;
  uint32_t lo = 0, hi = a.n_pass;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.work[mid] < w) lo = mid + 1; else hi = mid;
  }
  a.woff[w] = lo;
}

// kPlace false: medium and large works of this workgroup's 256 works into bcnt; true: the
// works to their lists, bcnt holding the two scans
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_rt_bin(RtArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t c = w < a.n_works ? a.woff[w + 1] - a.woff[w] : 0u;
  const bool medium = c > a.small && c <= a.lds, large = c > a.small && c > a.lds;
  uint32_t rm, tm, rl, tl;
  block_rank<kBlock>(medium, s_w, &rm, &tm);
  block_rank<kBlock>(large, s_w, &rl, &tl);
  if (!kPlace) {
    if (threadIdx.x == 0) {
      a.bcnt[blockIdx.x] = tm;
      a.bcnt[a.work_blocks + blockIdx.x] = tl;
    }
    if (medium) atomicMax(&a.status[kStMaxMedium], c);
  } else {
    if (medium) a.list[a.bcnt[blockIdx.x] + rm] = w;
    if (large) a.list[a.status[kStMedium] + a.bcnt[a.work_blocks + blockIdx.x] + rl] = w;
  }
}

__device__ inline uint64_t key_of(uint32_t best, uint32_t j) {
  return (uint64_t)best << 32 | (uint32_t)~j;
}

// a lane per work of 1 .. small passages: the recurrence as it stands
__global__ __launch_bounds__(kBlock) void k_rt_chain_small(RtArgs a) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= a.n_works) return;
  const uint32_t b = a.woff[w], c = a.woff[w + 1] - b;
  if (c == 0 || c > a.small) return;
  uint64_t end = 0;
  uint32_t words = 0, desc = 0;
  for (uint32_t i = 0; i < c; ++i) {
    const uint32_t ofi = a.of[b + i], nwi = a.nw[b + i];
    uint64_t key = 0;
    for (uint32_t j = 0; j < i; ++j) {
      const uint64_t cand = key_of(ld_agent(a.best + b + j), j);
      if (ofi > a.ol[b + j] && cand > key) key = cand;
    }
    const uint32_t j = ~(uint32_t)key;
    const uint32_t bi = nwi + (uint32_t)(key >> 32);
    st_agent(a.best + b + i, bi);
    a.prev[b + i] = key ? b + j : FS_NONE;
    st_agent(a.depth + b + i, key ? ld_agent(a.depth + b + j) + 1 : 1u);
    if (key_of(bi, i) > end) end = key_of(bi, i);
    words += nwi;
    desc += i && ofi <= a.ol[b + i - 1] ? 1u : 0u;
  }
  a.wend[w] = b + ~(uint32_t)end;
  a.wdesc[w] = desc;
  a.wwords[w] = words;
}

// a wave (= a workgroup) per listed work.  kLds: {orig_last, best, depth} of the work's
// passages in dynamic LDS (cap entries each), else read back from global memory.
template <bool kLds>
__global__ __launch_bounds__(64) void k_rt_chain_wave(RtArgs a, uint32_t list_first, uint32_t cap) {
  extern __shared__ uint32_t s_mem[];
  uint32_t* s_ol = s_mem;
  uint32_t* s_best = s_mem + cap;
  uint32_t* s_depth = s_mem + 2 * (size_t)cap;
  const uint32_t lane = threadIdx.x;
  const uint32_t w = a.list[list_first + blockIdx.x];
  const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.woff[w]);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.woff[w + 1]) - b;
  if (kLds && c > cap) return;                       // (the bins never list such a work here)
  uint64_t end = 0;
  uint32_t words = 0, desc = 0;
  for (uint32_t t0 = 0; t0 < c; t0 += 64) {
    const uint32_t i = t0 + lane;
    const bool live = i < c;
    const uint32_t myof = live ? a.of[b + i] : 0u;   // 0 follows nothing: a dead lane stays at key 0
    const uint32_t myol = live ? a.ol[b + i] : 0u;
    const uint32_t mynw = live ? a.nw[b + i] : 0u;
    uint64_t key = 0;
    // the earlier tiles, whole ones: 64 candidates per load
    for (uint32_t jt = 0; jt < t0; jt += 64) {
      const uint32_t o = kLds ? s_ol[jt + lane] : a.ol[b + jt + lane];
      const uint32_t v = kLds ? s_best[jt + lane] : ld_agent(a.best + b + jt + lane);
      for (uint32_t s = 0; s < 64; ++s) {
        const uint64_t cand = key_of(lane_u32(v, s), jt + s);
        if (myof > lane_u32(o, s) && cand > key) key = cand;
      }
    }
    uint32_t kdepth = 0;                             // depth of the candidate held in key
    if (key) {
      const uint32_t j = ~(uint32_t)key;
      kdepth = kLds ? s_depth[j] : ld_agent(a.depth + b + j);
    }
    // this tile: lane s is final once the steps before s are taken
    const uint32_t m = c - t0 < 64 ? c - t0 : 64u;
    for (uint32_t s = 0; s < m; ++s) {
      const uint32_t bs = lane_u32(mynw + (uint32_t)(key >> 32), s);
      const uint32_t os = lane_u32(myol, s);
      const uint32_t ds = lane_u32(kdepth + 1, s);
      const uint64_t cand = key_of(bs, t0 + s);
      if (lane > s && myof > os && cand > key) {
        key = cand;
        kdepth = ds;
      }
    }
    if (live) {
      const uint32_t mybest = mynw + (uint32_t)(key >> 32);
      a.prev[b + i] = key ? b + ~(uint32_t)key : FS_NONE;
      if (kLds) {
        s_ol[i] = myol;
        s_best[i] = mybest;
        s_depth[i] = kdepth + 1;
        a.best[b + i] = mybest;
        a.depth[b + i] = kdepth + 1;
      } else {
        st_agent(a.best + b + i, mybest);
        st_agent(a.depth + b + i, kdepth + 1);
      }
      if (key_of(mybest, i) > end) end = key_of(mybest, i);
      words += mynw;
      desc += i && myof <= a.ol[b + i - 1] ? 1u : 0u;
    }
    if (kLds) __syncthreads(); else __threadfence();  // the tile's values before the next reads them
  }
  end = wave_max(end);
  words = wave_sum(words);
  desc = wave_sum(desc);
  if (lane == 0) {
    a.wend[w] = b + ~(uint32_t)end;
    a.wdesc[w] = desc;
    a.wwords[w] = words;
  }
}

__device__ inline fs_retelling retelling_none() {
  return fs_retelling{0u, 0u, 0u, 0u, FS_NONE, FS_NONE, 0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(kBlock) void k_rt_none(fs_retelling* out, uint32_t n_works) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < n_works) out[w] = retelling_none();
}

__global__ __launch_bounds__(kBlock) void k_rt_trace(RtArgs a) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= a.n_works) return;
  const uint32_t b = a.woff[w], c = a.woff[w + 1] - b;
  if (!c) {
    a.out[w] = retelling_none();
    return;
  }
  const uint32_t end = a.wend[w];
  uint32_t script = 0, head = end;
  for (uint32_t i = end; i != FS_NONE; i = a.prev[i]) {
    a.cpos[i] = a.depth[i];
    script += a.ol[i] - a.of[i] + 1;
    head = i;
  }
  a.out[w] = fs_retelling{c, a.wwords[w], a.depth[end], a.best[end], head, end, a.of[head],
                          a.ol[end], script, a.wdesc[w]};
}

__global__ __launch_bounds__(kBlock) void k_rt_write(RtArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n_pass) return;
  a.passages[p] = fs_retelling_passage{a.first[p], a.nw[p], a.work[p], a.ff[p], a.fl[p], a.of[p],
                                       a.ol[p], a.best[p], a.prev[p], a.depth[p], a.cpos[p]};
}

// passages, bins, chains, trace, write, total of the last call
thread_local double t_ms[6];

struct RtScratch {
  DBuf<uint32_t> status, cnt, pass, woff, wres, bcnt, list;
  fs_runs* runs = nullptr;
  ~RtScratch() { if (runs) fs_runs_free(runs); }
};

// the rules both entry points share
int rt_check(uint64_t n_rows, uint32_t n_works, uint32_t min_words, const void* out,
             const void* passages, uint64_t cap, uint64_t* n_passages) {
  if (!n_passages || (n_works && !out) || (cap && !passages)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: retellings take fewer than 2^32", (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  *n_passages = 0;
  return FS_OK;
}

int rt_invalid() {
  fs_set_error("a work >= n_works");
  return FS_E_INVALID;
}

// d_out written and *n_passages set; d_passages too unless FS_E_CAPACITY (all on `s`, finished
// on return).
int rt_run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t min_words, uint32_t max_gap,
           fs_retelling* d_out, fs_retelling_passage* d_passages, uint64_t cap,
           uint64_t* n_passages, hipStream_t s) {
  for (double& t : t_ms) t = 0.0;
  if (n && !n_works) return rt_invalid();
  const RowsSrc src{d_rows};
  const dim3 blk(kBlock), work_grid(blocks_of(n_works, kBlock));
  const auto none = [&]() -> int {
    if (n_works) hipLaunchKernelGGL(k_rt_none, work_grid, blk, 0, s, d_out, n_works);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  };
  if (!n) return none();

  RtScratch k;
  RtArgs a{};
  Clock<6> clk;
  a.n = n;
  a.n_works = n_works;
  a.min_words = min_words;
  // FS_RETELLINGS_SMALL, FS_RETELLINGS_LDS: diagnostics, read on each call
  a.small = env_u32("FS_RETELLINGS_SMALL", kSmallDefault, 0xFFFFFFFFu);
  a.lds = env_u32("FS_RETELLINGS_LDS", kLdsDefault, kLdsMax);
  a.work_blocks = work_grid.x;
  a.out = d_out;
  a.passages = d_passages;
  FS_TRY(k.status.reserve(kStWords));
  FS_HIP(hipMemsetAsync(k.status.p, 0, kStWords * sizeof(uint32_t), s));
  a.status = k.status.p;
  FS_TRY(clk.mark(0, s));
  hipLaunchKernelGGL(k_rt_check, dim3(blocks_of(n, kBlock)), blk, 0, s, src, a);
  FS_HIP(hipGetLastError());
  FS_TRY(fs_runs_find(d_rows, n, min_words, max_gap, s, &k.runs, &a.heads, &a.n_runs));
  uint32_t st[kStWords];
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[kStBad]) return rt_invalid();

  // the kept runs, in record order
  const uint32_t run_blocks = blocks_of(a.n_runs, kBlock);
  FS_TRY(k.cnt.reserve(run_blocks));
  a.cnt = k.cnt.p;
  hipLaunchKernelGGL((k_rt_kept<false>), dim3(run_blocks), blk, 0, s, src, a);
  hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(kScanBlock), 0, s, a.cnt, a.cnt, run_blocks,
                     a.status + kStTotal);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  a.n_pass = st[kStTotal];
  *n_passages = a.n_pass;
  if (!a.n_pass) return none();
  const size_t np = a.n_pass;
  FS_TRY(k.pass.reserve(11 * np));
  FS_TRY(k.woff.reserve((size_t)n_works + 1));
  FS_TRY(k.wres.reserve(3 * (size_t)n_works));
  FS_TRY(k.bcnt.reserve(2 * (size_t)a.work_blocks));
  FS_TRY(k.list.reserve(n_works));
  a.first = k.pass.p;
  a.nw = k.pass.p + np;
  a.work = k.pass.p + 2 * np;
  a.ff = k.pass.p + 3 * np;
  a.fl = k.pass.p + 4 * np;
  a.of = k.pass.p + 5 * np;
  a.ol = k.pass.p + 6 * np;
  a.best = k.pass.p + 7 * np;
  a.prev = k.pass.p + 8 * np;
  a.depth = k.pass.p + 9 * np;
  a.cpos = k.pass.p + 10 * np;
  a.woff = k.woff.p;
  a.wend = k.wres.p;
  a.wdesc = k.wres.p + n_works;
  a.wwords = k.wres.p + 2 * (size_t)n_works;
  a.bcnt = k.bcnt.p;
  a.list = k.list.p;
  FS_HIP(hipMemsetAsync(a.cpos, 0, np * sizeof(uint32_t), s));
  hipLaunchKernelGGL((k_rt_kept<true>), dim3(run_blocks), blk, 0, s, src, a);
  hipLaunchKernelGGL(k_rt_offsets, dim3(blocks_of((uint64_t)n_works + 1, kBlock)), blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(1, s));

  // the works by class
  hipLaunchKernelGGL(k_rt_bin<false>, work_grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(kScanBlock), 0, s, a.bcnt, a.bcnt, a.work_blocks,
                     a.status + kStMedium);
  hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(kScanBlock), 0, s, a.bcnt + a.work_blocks,
                     a.bcnt + a.work_blocks, a.work_blocks, a.status + kStLarge);
  hipLaunchKernelGGL(k_rt_bin<true>, work_grid, blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  const uint32_t n_medium = st[kStMedium], n_large = st[kStLarge], cap_lds = st[kStMaxMedium];
  FS_TRY(clk.mark(2, s));

  // the chains
  if (a.small) hipLaunchKernelGGL(k_rt_chain_small, work_grid, blk, 0, s, a);
  if (n_medium)
    hipLaunchKernelGGL(k_rt_chain_wave<true>, dim3(n_medium), dim3(64),
                       3 * (size_t)cap_lds * sizeof(uint32_t), s, a, 0u, cap_lds);
  if (n_large)
    hipLaunchKernelGGL(k_rt_chain_wave<false>, dim3(n_large), dim3(64), 0, s, a, n_medium, 0u);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(3, s));
  hipLaunchKernelGGL(k_rt_trace, work_grid, blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, s));
  const bool fits = a.n_pass <= cap;
  if (fits) hipLaunchKernelGGL(k_rt_write, dim3(blocks_of(np, kBlock)), blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(5, s));
  FS_HIP(hipStreamSynchronize(s));
  for (int j = 0; j < 5; ++j) t_ms[j] = clk.elapsed(j, j + 1);
  t_ms[5] = clk.elapsed(0, 5);
  if (!fits) {
    fs_set_error("%u passages need room", a.n_pass);
    return FS_E_CAPACITY;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_retellings(int device, const uint32_t* work, const uint32_t* fan_ix,
                             const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                             uint32_t min_words, uint32_t max_gap, fs_retelling* out,
                             fs_retelling_passage* passages, uint64_t cap,
                             uint64_t* n_passages) {
  FS_TRY(rt_check(n_rows, n_works, min_words, out, passages, cap, n_passages));
  if (!n_rows) {
    const fs_retelling none{0u, 0u, 0u, 0u, FS_NONE, FS_NONE, 0u, 0u, 0u, 0u};
    for (uint32_t w = 0; w < n_works; ++w) out[w] = none;
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
  DBuf<fs_retelling> d_out;
  DBuf<fs_retelling_passage> d_pass;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_out.reserve(n_works));
  const uint64_t most = n_rows / min_words;                  // passages never outnumber this
  FS_TRY(d_pass.reserve(cap < most ? cap : most));
  const int rc = rt_run(rows.p, n, n_works, min_words, max_gap, d_out.p, d_pass.p, cap, n_passages,
                        nullptr);
  if (rc != FS_OK && rc != FS_E_CAPACITY) return rc;
  if (n_works) FS_TRY(copy_out(out, d_out, n_works));
  if (rc == FS_OK && *n_passages) FS_TRY(copy_out(passages, d_pass, *n_passages));
  FS_HIP(hipDeviceSynchronize());
  return rc;
}

extern "C" int fs_retellings_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                  uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                                  fs_retelling* d_out, fs_retelling_passage* d_passages,
                                  uint64_t cap, uint64_t* n_passages) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_TRY(rt_check(n_rows, n_works, min_words, d_out, d_passages, cap, n_passages));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_out & 3) ||
      ((uintptr_t)d_passages & 7)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_passages 8-byte, d_out 4-byte");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  return rt_run(d_rows, (uint32_t)n_rows, n_works, min_words, max_gap, d_out, d_passages, cap,
                n_passages, ix->stream);
}

extern "C" int fs_retellings_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
