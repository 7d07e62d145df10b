// fs_pairs.hip -- `ao3.py pairs`: fan works related by the script words both quote (fs_pairs,
// fs_pairs_rows in include/fandom_search.h).  The coverage of a work is a row of bits over the
// script; a pair's shared words are the popcount of the AND of two rows.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   fs_runs_find     the run heads of fs_passages.hip (and its sortedness check)
//   k_pairs_check    one lane per record: a work >= n_works, an orig_ix >= n_script
//   k_pairs_flag     one lane per run: a kept run flags its work as active
//   k_pairs_scan     one workgroup: active works numbered in work order; later the offsets
//   k_pairs_list     one lane per work: the work of an active number
//   k_pairs_cover    one lane per run: a kept run's span ORed into its work's row, a 64-bit
//                    word at a time
//   k_pairs_covered  one lane per active work: the popcount of its row
//   k_pairs_tiles<0> the count pass.  A workgroup takes a row tile of 64 active works and a
//                    chunk of kChunk column tiles from the upper triangle; per column tile it
//                    walks the script in K-slices staged in LDS, every thread a 4 x 4 block of
//                    pair counts; kept pairs per (row, chunk), partners and best of both works
//   k_pairs_scan     offsets in (row, chunk) order: the pairs come out in (a, b) order
//   k_pairs_works    one lane per work: its fs_pair_work
//   k_pairs_tiles<1> the place pass: the column tiles that keep a pair computed again, in
//                    order, each row's kept pairs placed behind its cursor in ascending b
//   k_pairs_detail   one lane per kept pair: first, last and the longest run of the AND
//
// The passes up to the row popcounts and the tile product (tile_counts) live in fs_tiles.h,
// with the layout of the matrix, and are shared with fs_clusters.hip.  The detail pass reads
// neighbouring pairs, same a and adjacent b, from adjacent addresses.
#include "fs_tiles.h"

namespace {

struct PairsArgs : CoverArgs {
  uint32_t* partners;           // [n_tiles * 64]
  unsigned long long* best;     // [n_tiles * 64] shared << 32 | (0xFFFFFFFF - partner)
  uint32_t* cnt;                // [n_tiles * 64][n_chunks] kept pairs of a row in a chunk
  unsigned long long* off;      // the same, scanned
  uint32_t* any;                // [n_tiles][n_chunks] bit t: column tile t of the chunk keeps a pair
  unsigned long long* total;    // kept pairs
  fs_pair_work* works;
  fs_pair* pairs;
};

// blockIdx.x = row tile * n_chunks + chunk.  kPlace 0: counts, partners, best; 1: the pairs.
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_pairs_tiles(PairsArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ uint32_t s_wa[kTile], s_wb[kTile], s_rowcnt[kTile];
  __shared__ unsigned long long s_cur[kTile];
  __shared__ uint32_t s_any;
  const uint32_t ti = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const uint32_t tj0 = ti > c * kChunk ? ti : c * kChunk;
  const uint32_t tj1 = (c + 1) * kChunk < a.n_tiles ? (c + 1) * kChunk : a.n_tiles;
  if (tj0 >= tj1) return;                                // below the diagonal
  const uint32_t mask = kPlace ? a.any[blockIdx.x] : 0u;
  if (kPlace && !mask) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kTile) {
    s_wa[threadIdx.x] = a.work_of[(size_t)ti * kTile + threadIdx.x];
    s_rowcnt[threadIdx.x] = 0;
    if (kPlace)
      s_cur[threadIdx.x] = a.off[((size_t)ti * kTile + threadIdx.x) * a.n_chunks + c];
  }
  if (threadIdx.x == 0) s_any = 0;
  for (uint32_t tj = tj0; tj < tj1; ++tj) {
    if (kPlace && !((mask >> (tj - c * kChunk)) & 1)) continue;
    __syncthreads();                                     // s_wb and s_sh of the tile before
    if (threadIdx.x < kTile) s_wb[threadIdx.x] = a.work_of[(size_t)tj * kTile + threadIdx.x];
    tile_counts(a, ti, tj, s_a, s_b, s_sh);
    const bool diag = tj == ti;
    // rows: wave w takes rows 16 w .. 16 w + 15, a lane per column
    bool kept_any = false;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const bool keep = sh >= a.min_shared && (!diag || r < lane);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      kept_any = true;
      const uint32_t cn = (uint32_t)__popcll(m);
      if (kPlace) {
        const unsigned long long pos = s_cur[r] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (keep) {
          uint4* p = reinterpret_cast<uint4*>(a.pairs + pos);
          p[0] = make_uint4(s_wa[r], s_wb[lane], sh, 0u);
          p[1] = make_uint4(0u, 0u, 0u, 0u);
        }
        if (lane == 0) s_cur[r] += cn;
      } else {
        const unsigned long long key =
            wave_max(keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - s_wb[lane]) : 0ull);
        if (lane == 0) {
          s_rowcnt[r] += cn;
          atomicAdd(&a.partners[(size_t)ti * kTile + r], cn);
          atomicMax(&a.best[(size_t)ti * kTile + r], key);
        }
      }
    }
    if (kPlace) continue;
    if (kept_any && lane == 0) atomicOr(&s_any, 1u << (tj - c * kChunk));
    // columns: wave w takes columns 16 w .. 16 w + 15, a lane per row
    if (!__syncthreads_or(kept_any)) continue;
    for (uint32_t cc = 0; cc < kTile / 4; ++cc) {
      const uint32_t col = wave * (kTile / 4) + cc;
      const uint32_t sh = s_sh[lane * kShStride + col];
      const bool keep = sh >= a.min_shared && (!diag || lane < col);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      const unsigned long long key =
          wave_max(keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - s_wa[lane]) : 0ull);
      if (lane == 0) {
        atomicAdd(&a.partners[(size_t)tj * kTile + col], (uint32_t)__popcll(m));
        atomicMax(&a.best[(size_t)tj * kTile + col], key);
      }
    }
  }
  if (kPlace) return;
  __syncthreads();
  if (threadIdx.x < kTile)
    a.cnt[((size_t)ti * kTile + threadIdx.x) * a.n_chunks + c] = s_rowcnt[threadIdx.x];
  if (threadIdx.x == 0) a.any[blockIdx.x] = s_any;
}

// one lane per work
__global__ __launch_bounds__(kRunBlock) void k_pairs_works(PairsArgs a, const uint32_t* flag) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.n_works) return;
  uint4 o = make_uint4(0u, 0u, FS_NONE, 0u);
  if (flag && flag[w]) {
    const uint32_t ai = a.act[w];
    const unsigned long long b = a.best[ai];
    o.x = a.covered[ai];
    o.y = a.partners[ai];
    if (o.y) {
      o.z = 0xFFFFFFFFu - (uint32_t)b;
      o.w = (uint32_t)(b >> 32);
    }
  }
  reinterpret_cast<uint4*>(a.works)[w] = o;
}

// One lane per kept pair: what its two rows share (shared_run, fs_tiles.h).
__global__ __launch_bounds__(kRunBlock) void k_pairs_detail(PairsArgs a, uint64_t n_pairs) {
  const uint64_t p = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (p >= n_pairs) return;
  const uint4 head = reinterpret_cast<const uint4*>(a.pairs + p)[0];
  const uint32_t ia = a.act[head.x], ib = a.act[head.y];
  const SharedRun r = shared_run(a.cov + (size_t)(ia / kTile) * a.nk * kTile + ia % kTile,
                                 a.cov + (size_t)(ib / kTile) * a.nk * kTile + ib % kTile, a.nk);
  reinterpret_cast<uint4*>(a.pairs + p)[1] = make_uint4(r.last, r.run_first, r.run_words, 0u);
  a.pairs[p].first = r.first;
}

thread_local double t_ms[4];    // coverage, count, place, detail of the last call

// one call: count() through the per-work results and the number of pairs, then write()
struct PairsJob {
  CoverJob cj;
  DBuf<uint32_t> partners, cnt, any;
  DBuf<unsigned long long> best, off, total;
  Clock<8> clk;
  PairsArgs a{};
  uint64_t n_pairs = 0;

  // d_works written, n_pairs set (all on `s`, finished on return)
  int count(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
            uint32_t min_words, uint32_t max_gap, uint32_t min_shared, fs_pair_work* d_works,
            hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.min_shared = min_shared;
    a.works = d_works;
    const dim3 work_grid((n_works + kRunBlock - 1) / kRunBlock), blk(kRunBlock);
    if (n) FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) {
      if (n_works) hipLaunchKernelGGL(k_pairs_works, work_grid, blk, 0, s, a, nullptr);
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));
      return FS_OK;
    }
    if ((uint64_t)a.n_active * a.nk * 8 > FS_PAIRS_MAX_BYTES) {
      fs_set_error("%u works with a passage over %u script words: a coverage matrix of more "
                   "than %u bytes", a.n_active, n_script, FS_PAIRS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    const size_t rows = (size_t)a.n_tiles * kTile, cells = rows * a.n_chunks;
    const uint64_t blocks = (uint64_t)a.n_tiles * a.n_chunks;
    if (blocks > 0x7FFFFFFFull) {
      fs_set_error("%u works with a passage: more tiles of pairs than a launch takes",
                   a.n_active);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(cj.reserve(a, s));
    FS_TRY(partners.reserve(rows));
    FS_TRY(best.reserve(rows));
    FS_TRY(cnt.reserve(cells));
    FS_TRY(off.reserve(cells));
    FS_TRY(any.reserve((size_t)blocks));
    FS_TRY(total.reserve(1));
    FS_HIP(hipMemsetAsync(partners.p, 0, rows * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(best.p, 0, rows * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(cnt.p, 0, cells * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(any.p, 0, (size_t)blocks * sizeof(uint32_t), s));
    a.partners = partners.p;
    a.best = best.p;
    a.cnt = cnt.p;
    a.off = off.p;
    a.any = any.p;
    a.total = total.p;
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    FS_TRY(clk.mark(1, s));
    hipLaunchKernelGGL(k_pairs_tiles<0>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s, cnt.p,
                       (uint64_t)cells, off.p, total.p);
    hipLaunchKernelGGL(k_pairs_works, work_grid, blk, 0, s, a, cj.flag.p);
    FS_TRY(clk.mark(2, s));
    FS_HIP(hipGetLastError());
    unsigned long long tot = 0;
    FS_HIP(hipMemcpyAsync(&tot, total.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    n_pairs = tot;
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    return FS_OK;
  }

  // the n_pairs pairs into d_pairs (finished on return)
  int write(fs_pair* d_pairs, hipStream_t s) {
    if (!n_pairs) return FS_OK;
    a.pairs = d_pairs;
    FS_TRY(clk.mark(3, s));
    hipLaunchKernelGGL(k_pairs_tiles<1>, dim3(a.n_tiles * a.n_chunks), dim3(kBlock), 0, s, a);
    FS_TRY(clk.mark(4, s));
    hipLaunchKernelGGL(k_pairs_detail, dim3((uint32_t)((n_pairs + kRunBlock - 1) / kRunBlock)),
                       dim3(kRunBlock), 0, s, a, (uint64_t)n_pairs);
    FS_TRY(clk.mark(5, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[2] = clk.elapsed(3, 4);
    t_ms[3] = clk.elapsed(4, 5);
    return FS_OK;
  }
};

// the rules both entry points share
int pairs_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
                uint32_t min_shared, const void* works, const void* pairs, uint64_t cap,
                uint64_t* n_pairs) {
  if (!n_pairs || (n_works && !works) || (cap && !pairs)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_shared == 0) {
    fs_set_error("min_words and min_shared must be at least 1");
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("pairs", n_rows, n_script));
  *n_pairs = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_pairs(int device, const uint32_t* work, const uint32_t* fan_ix,
                        const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                        uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                        uint32_t min_shared, fs_pair_work* works, fs_pair* pairs, uint64_t cap,
                        uint64_t* n_pairs) {
  FS_TRY(pairs_check(n_rows, n_works, n_script, min_words, min_shared, works, pairs, cap,
                     n_pairs));
  if (!n_rows) {
    const fs_pair_work none{0u, 0u, FS_NONE, 0u};
    for (uint32_t w = 0; w < n_works; ++w) works[w] = none;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_pair_work> d_works;
  DBuf<fs_pair> d_pairs;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_works.reserve(n_works));
  PairsJob job;
  FS_TRY(job.count(rows.p, n, n_works, n_script, min_words, max_gap, min_shared, d_works.p,
                   nullptr));
  if (n_works) FS_TRY(copy_out(works, d_works, n_works));
  *n_pairs = job.n_pairs;
  if (job.n_pairs > cap) return FS_E_CAPACITY;
  if (job.n_pairs) {
    FS_TRY(d_pairs.reserve(job.n_pairs));
    FS_TRY(job.write(d_pairs.p, nullptr));
    FS_TRY(copy_out(pairs, d_pairs, job.n_pairs));
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_pairs_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                             uint32_t min_words, uint32_t max_gap, uint32_t min_shared,
                             fs_pair_work* d_works, fs_pair* d_pairs, uint64_t cap,
                             uint64_t* n_pairs) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: pairs take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(pairs_check(n_rows, n_works, (uint32_t)ix->n_script, min_words, min_shared, d_works,
                     d_pairs, cap, n_pairs));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_works & 15) ||
      ((uintptr_t)d_pairs & 15)) {
    fs_set_error("d_rows, d_works and d_pairs must be 16-byte aligned device pointers");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  PairsJob job;
  FS_TRY(job.count(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                   min_shared, d_works, ix->stream));
  *n_pairs = job.n_pairs;
  if (job.n_pairs > cap) return FS_E_CAPACITY;
  return job.write(d_pairs, ix->stream);
}

extern "C" int fs_pairs_times(double* ms) {
  return times_out(ms, t_ms, 4);
}
