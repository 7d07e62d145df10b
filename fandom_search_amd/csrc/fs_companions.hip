// fs_companions.hip -- `ao3.py companions`: stretches of the script related by the fan works
// that quote both (fs_companions, fs_companions_rows in include/fandom_search.h).  The transpose
// of fs_pairs.hip: a unit (a quoted region, a scene, a character) is a row of bits over the
// active works, the incidence matrix M; a pair's common works are the popcount of the AND of two
// rows.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   incidence        IncJob of fs_incidence.h, which the other units over M share:
//   k_comp_units_ok  one lane per script word: a unit number that is neither < n_units nor none
//   CoverJob::number the run heads, the check of every record, the active works numbered
//   k_pairs_list     one lane per work: the work of an active number
//   k_comp_incidence a lane per run finds the kept ones; the wave then takes them one at a time,
//                    its lanes striding the run's span: the work's bit ORed into the row of the
//                    unit at the span's first word and at every word whose unit differs from the
//                    word before.  The coverage matrix of `pairs` is never built
//   k_pairs_covered  works(u), the popcount of row u
//   k_comp_tiles<0>  the count pass: k_pairs_tiles<0> over M with the keep rule of both and share
//   k_pairs_scan     offsets in (row, chunk) order: the pairs come out in (a, b) order
//   k_comp_units     one lane per unit: its fs_companion_unit
//   k_comp_tiles<1>  the place pass
//   k_comp_detail    one lane per kept pair: the first and the last work of the AND
//
// M is stored as fs_tiles.h stores the coverage matrix, [tile of 64 units][k][64] with k over
// the 64-bit words of the active works, so tile_counts runs on it through a CoverArgs whose cov,
// nk and n_tiles describe M.  Rows past n_units are zero and are never kept (min_both >= 1).
// k_comp_units_ok, k_comp_incidence and the host sequence around them live in fs_incidence.h.
#include "fs_incidence.h"

namespace {

struct CompArgs : IncArgs {     // r, m, unit_of, n_units: fs_incidence.h
  uint32_t min_both, min_share;
  uint32_t* partners;           // [m.n_tiles * 64]
  unsigned long long* best;     // [m.n_tiles * 64] both << 32 | (0xFFFFFFFF - partner)
  uint32_t* cnt;                // [m.n_tiles * 64][n_chunks] kept pairs of a row in a chunk
  unsigned long long* off;      // the same, scanned
  uint32_t* any;                // [m.n_tiles][n_chunks] bit t: column tile t of the chunk keeps a pair
  unsigned long long* total;    // kept pairs
  fs_companion_unit* units;
  fs_companion* pairs;
};

// one lane per unit: a unit nobody quotes (no records, or no work with a passage)
__global__ __launch_bounds__(kRunBlock) void k_comp_units_none(fs_companion_unit* units,
                                                               uint32_t n_units) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u < n_units) reinterpret_cast<uint4*>(units)[u] = make_uint4(0u, 0u, FS_NONE, 0u);
}

__device__ inline bool comp_keep(const CompArgs& a, uint32_t both, uint32_t wa, uint32_t wb) {
  const uint32_t least = wa < wb ? wa : wb;
  return both >= a.min_both &&
         (unsigned long long)both * 100ull >= (unsigned long long)a.min_share * least;
}

// blockIdx.x = row tile * n_chunks + chunk.  kPlace 0: counts, partners, best; 1: the pairs.
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_comp_tiles(CompArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ uint32_t s_wa[kTile], s_wb[kTile], s_rowcnt[kTile];
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
    s_wa[threadIdx.x] = a.m.covered[(size_t)ti * kTile + threadIdx.x];
    s_rowcnt[threadIdx.x] = 0;
    if (kPlace) s_cur[threadIdx.x] = a.off[((size_t)ti * kTile + threadIdx.x) * n_chunks + c];
  }
  if (threadIdx.x == 0) s_any = 0;
  for (uint32_t tj = tj0; tj < tj1; ++tj) {
    if (kPlace && !((mask >> (tj - c * kChunk)) & 1)) continue;
    __syncthreads();                                     // s_wb and s_sh of the tile before
    if (threadIdx.x < kTile) s_wb[threadIdx.x] = a.m.covered[(size_t)tj * kTile + threadIdx.x];
    tile_counts(a.m, ti, tj, s_a, s_b, s_sh);
    const bool diag = tj == ti;
    // rows: wave w takes rows 16 w .. 16 w + 15, a lane per column
    bool kept_any = false;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const bool keep = comp_keep(a, sh, s_wa[r], s_wb[lane]) && (!diag || r < lane);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      kept_any = true;
      const uint32_t cn = (uint32_t)__popcll(m);
      if (kPlace) {
        const unsigned long long pos = s_cur[r] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (keep) {
          uint4* p = reinterpret_cast<uint4*>(a.pairs + pos);
          p[0] = make_uint4(ti * kTile + r, tj * kTile + lane, sh, s_wa[r]);
          p[1] = make_uint4(s_wb[lane], 0u, 0u, 0u);
        }
        if (lane == 0) s_cur[r] += cn;
      } else {
        const unsigned long long key = wave_max(
            keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - (tj * kTile + lane)) : 0ull);
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
      const bool keep = comp_keep(a, sh, s_wa[lane], s_wb[col]) && (!diag || lane < col);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      const unsigned long long key = wave_max(
          keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - (ti * kTile + lane)) : 0ull);
      if (lane == 0) {
        atomicAdd(&a.partners[(size_t)tj * kTile + col], (uint32_t)__popcll(m));
        atomicMax(&a.best[(size_t)tj * kTile + col], key);
      }
    }
  }
  if (kPlace) return;
  __syncthreads();
  if (threadIdx.x < kTile)
    a.cnt[((size_t)ti * kTile + threadIdx.x) * n_chunks + c] = s_rowcnt[threadIdx.x];
  if (threadIdx.x == 0) a.any[blockIdx.x] = s_any;
}

// one lane per unit
__global__ __launch_bounds__(kRunBlock) void k_comp_units(CompArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u >= a.n_units) return;
  const unsigned long long b = a.best[u];
  uint4 o = make_uint4(a.m.covered[u], a.partners[u], FS_NONE, 0u);
  if (o.y) {
    o.z = 0xFFFFFFFFu - (uint32_t)b;
    o.w = (uint32_t)(b >> 32);
  }
  reinterpret_cast<uint4*>(a.units)[u] = o;
}

// One lane per kept pair: the AND of the two rows from the front up to its first set bit, from
// the back down to its last.  A kept pair has both >= 1, so both are found.
__global__ __launch_bounds__(kRunBlock) void k_comp_detail(CompArgs a, uint64_t n_pairs) {
  const uint64_t p = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (p >= n_pairs) return;
  const uint4 head = reinterpret_cast<const uint4*>(a.pairs + p)[0];
  const uint32_t wb = reinterpret_cast<const uint4*>(a.pairs + p)[1].x;
  const uint32_t nk = a.m.nk;
  const unsigned long long* ra = a.m.cov + (size_t)(head.x / kTile) * nk * kTile + head.x % kTile;
  const unsigned long long* rb = a.m.cov + (size_t)(head.y / kTile) * nk * kTile + head.y % kTile;
  uint32_t first = FS_NONE, last = FS_NONE;
  for (uint32_t k = 0; k < nk; ++k) {
    const unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    if (x) {
      first = k * 64 + (uint32_t)__builtin_ctzll(x);
      break;
    }
  }
  for (uint32_t k = nk; k-- > 0;) {
    const unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    if (x) {
      last = k * 64 + 63 - (uint32_t)__builtin_clzll(x);
      break;
    }
  }
  const uint32_t fw = first < a.r.n_active ? a.r.work_of[first] : FS_NONE;
  const uint32_t lw = last < a.r.n_active ? a.r.work_of[last] : FS_NONE;
  reinterpret_cast<uint4*>(a.pairs + p)[1] = make_uint4(wb, fw, lw, 0u);
}

thread_local double t_ms[4];    // incidence, count, place, detail of the last call

// one call: count() through the per-unit results and the number of pairs, then write()
struct CompJob {
  IncJob inc;
  DBuf<uint32_t> partners, cnt, any;
  DBuf<unsigned long long> best, off, total;
  Clock<8> clk;
  CompArgs a{};
  uint64_t n_pairs = 0;

  int none(hipStream_t s) {
    if (a.n_units)
      hipLaunchKernelGGL(k_comp_units_none, dim3((a.n_units + kRunBlock - 1) / kRunBlock),
                         dim3(kRunBlock), 0, s, a.units, a.n_units);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }

  // d_units written, n_pairs set (all on `s`, finished on return)
  int count(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
            const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
            uint32_t min_both, uint32_t min_share, fs_companion_unit* d_units, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.min_both = min_both;
    a.min_share = min_share;
    a.units = d_units;
    if (!n || !n_units) return none(s);
    FS_TRY(inc.number(d_rows, a, max_gap, s));
    if (!a.r.n_active) return none(s);
    if (IncJob::mat_bytes(a) > FS_COMPANIONS_MAX_BYTES) {
      fs_set_error("%u units over %u works with a passage: an incidence matrix of more than %u "
                   "bytes", n_units, a.r.n_active, FS_COMPANIONS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    const size_t rows = (size_t)a.m.n_tiles * kTile, cells = rows * a.m.n_chunks;
    const uint64_t blocks = (uint64_t)a.m.n_tiles * a.m.n_chunks;
    if (blocks > 0x7FFFFFFFull) {
      fs_set_error("%u units: more tiles of pairs than a launch takes", n_units);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(inc.reserve(a, true, s));
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
    const dim3 blk(kRunBlock);
    FS_TRY(clk.mark(0, s));
    inc.incidence(d_rows, a, s);
    FS_TRY(clk.mark(1, s));
    hipLaunchKernelGGL(k_comp_tiles<0>, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s, cnt.p,
                       (uint64_t)cells, off.p, total.p);
    hipLaunchKernelGGL(k_comp_units, dim3((n_units + kRunBlock - 1) / kRunBlock), blk, 0, s, a);
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
  int write(fs_companion* d_pairs, hipStream_t s) {
    if (!n_pairs) return FS_OK;
    a.pairs = d_pairs;
    FS_TRY(clk.mark(3, s));
    hipLaunchKernelGGL(k_comp_tiles<1>, dim3(a.m.n_tiles * a.m.n_chunks), dim3(kBlock), 0, s, a);
    FS_TRY(clk.mark(4, s));
    hipLaunchKernelGGL(k_comp_detail, dim3((uint32_t)((n_pairs + kRunBlock - 1) / kRunBlock)),
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
int comp_check(uint64_t n_rows, uint32_t n_script, const void* unit_of, uint32_t n_units,
               uint32_t min_words, uint32_t min_both, uint32_t min_share, const void* units,
               const void* pairs, uint64_t cap, uint64_t* n_pairs) {
  if (!n_pairs || (n_units && !units) || (cap && !pairs) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_both == 0) {
    fs_set_error("min_words and min_both must be at least 1");
    return FS_E_INVALID;
  }
  if (min_share > 100) {
    fs_set_error("min_share %u: a whole percentage, 0 to 100", min_share);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("companions", n_rows, n_script));
  *n_pairs = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_companions(int device, const uint32_t* work, const uint32_t* fan_ix,
                             const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                             uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                             uint32_t min_words, uint32_t max_gap, uint32_t min_both,
                             uint32_t min_share, fs_companion_unit* units, fs_companion* pairs,
                             uint64_t cap, uint64_t* n_pairs) {
  FS_TRY(comp_check(n_rows, n_script, unit_of, n_units, min_words, min_both, min_share, units,
                    pairs, cap, n_pairs));
  if (!n_rows || !n_units) {
    const fs_companion_unit none{0u, 0u, FS_NONE, 0u};
    for (uint32_t u = 0; u < n_units; ++u) units[u] = none;
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
  DBuf<fs_companion_unit> d_units;
  DBuf<fs_companion> d_pairs;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n_script, nullptr));
  FS_TRY(d_units.reserve(n_units));
  CompJob job;
  FS_TRY(job.count(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap,
                   min_both, min_share, d_units.p, nullptr));
  FS_TRY(copy_out(units, d_units, n_units));
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

extern "C" int fs_companions_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                  uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                                  uint32_t min_words, uint32_t max_gap, uint32_t min_both,
                                  uint32_t min_share, fs_companion_unit* d_units,
                                  fs_companion* d_pairs, uint64_t cap, uint64_t* n_pairs) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: companions take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(comp_check(n_rows, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, min_both,
                    min_share, d_units, d_pairs, cap, n_pairs));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 15) || ((uintptr_t)d_pairs & 15)) {
    fs_set_error("d_rows, d_units and d_pairs must be 16-byte aligned device pointers, "
                 "d_unit_of 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  CompJob job;
  FS_TRY(job.count(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                   min_words, max_gap, min_both, min_share, d_units, ix->stream));
  *n_pairs = job.n_pairs;
  if (job.n_pairs > cap) return FS_E_CAPACITY;
  return job.write(d_pairs, ix->stream);
}

extern "C" int fs_companions_times(double* ms) {
  return times_out(ms, t_ms, 4);
}
