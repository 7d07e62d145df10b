// fs_lines.hip -- `ao3.py lines`: the lines of the script by how completely the fan works quote
// them (fs_lines, fs_lines_rows in include/fandom_search.h).  `companions` asks whether a work
// touches a unit; this unit measures how much of a line a work covers: per cell (line, work)
// the covered words, the first and last of them and their runs.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   k_lines_check    one lane per entry of line_first: 0, strictly ascending, n_script
//   k_lines_map      one lane per script word: its line (a binary search that stays inside the
//                    table whatever the table holds)
//   CoverJob::number the run heads, the check of every record, the active works numbered
//   k_pairs_list     one lane per work: the work of an active number
//   k_lines_init     one lane per line: its fs_line cleared
//   k_lines_tables   a lane per run finds the kept ones; the wave then takes them one at a time:
//                    its lanes stride the span's 64-bit words (fs_cover_span, a word each) and
//                    then the lines the span enters, the work's bit ORed into each line's row
//   k_lines_popc     a wave per line: the cells of the line, and in front of each column of 64
//                    active works the cells of the columns before it
//   k_pairs_scan     the lines' offsets: the cells come out in (line, work) order
//   k_lines_walk     a wave per column and chunk of lines, a lane per work: the figures of every
//                    cell; per-line sums through LDS, per-work sums in registers; the cells
//                    written when the caller's buffers hold them
//   k_lines_works    one lane per active work: its fs_line_work
//
// The coverage is word-major: 64-bit word k of active work a is at cov[k * stride + a] with
// stride = the active works padded to 64, so the 64 lanes of a wave read word k of 64 works in
// one 512-byte access.  The incidence row of line l is inc[l * n_cols .. + n_cols), a bit per
// active work.  Columns past the last active work are zero in both and never count.
#include "fs_tiles.h"

namespace {

constexpr uint32_t kWalkWaves = 4;                    // columns a workgroup takes
constexpr uint32_t kWalkBlock = kWalkWaves * 64;
constexpr uint32_t kLinesChunkMax = 256;              // lines per chunk: the per-line sums in LDS
constexpr uint32_t kLinesChunkDefault = 16;            // short: a wave takes its lines in turn

struct LinesArgs {
  CoverArgs r;                  // the records: heads, act, work_of, n_active; cov word-major
  const uint32_t* line_first;   // [n_lines + 1]
  uint32_t n_lines, most, chunk, skip, n_cols, n_chunks;
  size_t stride;                // n_cols * 64
  uint32_t* line_of;            // [n_script]
  unsigned long long* inc;      // [n_lines][n_cols]
  uint32_t* pre;                // [n_lines][n_cols] cells of the line in the columns before
  uint32_t* cnt;                // [n_lines] cells of a line
  unsigned long long* off;      // the same, scanned
  unsigned long long* total;    // cells
  uint32_t* wacc;               // [4][stride] lines, whole_lines, covered, line_words
  unsigned long long* wtop;     // [stride] covered << 32 | ~line
  fs_line* lines;
  fs_line_work* works;
  fs_line_cell* cells;
};

// one lane per entry of line_first
__global__ __launch_bounds__(kRunBlock) void k_lines_check(const uint32_t* line_first,
                                                           uint32_t n_lines, uint32_t n_script,
                                                           uint32_t* bad_out) {
  const uint64_t l = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  bool bad = false;
  if (l <= n_lines) {
    const uint32_t at = line_first[l];
    if (l == 0 && at != 0) bad = true;
    if (l == n_lines ? at != n_script : at >= line_first[l + 1]) bad = true;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(bad_out, 1u);
}

// one lane per script word: the last line that starts at or before it (n_lines >= 1; every
// read is of line_first[0 .. n_lines - 1], whatever the table holds)
__global__ __launch_bounds__(kRunBlock) void k_lines_map(const uint32_t* line_first,
                                                         uint32_t n_lines, uint32_t n_script,
                                                         uint32_t* line_of) {
  const uint64_t o = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (o >= n_script) return;
  uint32_t lo = 0, hi = n_lines - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (line_first[mid] <= o) lo = mid; else hi = mid - 1;
  }
  line_of[o] = lo;
}

// one lane per line: nobody quotes it (yet)
__global__ __launch_bounds__(kRunBlock) void k_lines_init(fs_line* lines, uint32_t n_lines) {
  const uint64_t l = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (l >= n_lines) return;
  uint4* p = reinterpret_cast<uint4*>(lines + l);
  p[0] = make_uint4(0u, 0u, 0u, 0u);
  p[1] = make_uint4(0u, FS_NONE, 0u, 0u);
}

// A lane per run (after CoverJob::number found nothing: every work and word is inside, and
// k_lines_check: line_of is the line of every word); the wave's kept runs are then taken in
// turn by the whole wave.
__global__ __launch_bounds__(kRunBlock) void k_lines_tables(RowsSrc src, LinesArgs a,
                                                            const uint32_t* flag) {
  const uint64_t r = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  bool kept = false;
  uint32_t o0 = 0, o1 = 0, ai = 0;
  if (r < a.r.n_runs) {
    const uint32_t h = a.r.heads[r], e = a.r.heads[r + 1];
    if (e - h >= a.r.min_words) {
      const uint4 k = src.key(h);
      o0 = k.z;
      o1 = src.key((uint64_t)e - 1).z;                       // o0 <= o1: a run steps forward
      if (k.x < a.r.n_works && flag[k.x] && o1 < a.r.n_script && o0 <= o1) {
        kept = true;
        ai = a.r.act[k.x];
      }
    }
  }
  uint64_t todo = __ballot(kept);
  while (todo) {
    const int from = __builtin_ctzll(todo);
    todo &= todo - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)o0, from), b1 = (uint32_t)__shfl((int)o1, from);
    const uint32_t bi = (uint32_t)__shfl((int)ai, from);
    if (bi >= a.r.n_active) continue;                      // (never: act numbers the flagged works)
    // the coverage: a lane per 64-bit word of the span
    for (uint32_t k = (b0 >> 6) + lane; k <= (b1 >> 6); k += 64) {
      const uint32_t lo = k << 6, hi = lo + 63;
      fs_cover_span(a.r.cov + bi, a.stride, b0 > lo ? b0 : lo, b1 < hi ? b1 : hi);
    }
    // the incidence: a lane per line the span enters
    const uint32_t l0 = a.line_of[b0], l1 = a.line_of[b1];
    const unsigned long long bit = 1ull << (bi & 63);
    for (uint64_t l = (uint64_t)l0 + lane; l <= l1; l += 64)
      atomicOr(&a.inc[l * a.n_cols + (bi >> 6)], bit);
  }
}

// a wave per line, its lanes striding the columns
__global__ __launch_bounds__(kRunBlock) void k_lines_popc(LinesArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t l = (uint64_t)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (l >= a.n_lines) return;                              // (wave-uniform)
  uint32_t before = 0;
  for (uint32_t c0 = 0; c0 < a.n_cols; c0 += 64) {
    const uint32_t c = c0 + lane;
    const size_t at = (size_t)l * a.n_cols + c;
    const uint32_t x = c < a.n_cols ? (uint32_t)__popcll(a.inc[at]) : 0u;
    const uint32_t upto = wave_scan(x);
    if (c < a.n_cols) a.pre[at] = before + upto - x;
    before += lane_u32(upto, 63);
  }
  if (lane == 0) a.cnt[l] = before;
}

// blockIdx.x = group of kWalkWaves columns * n_chunks + chunk; wave w takes column group *
// kWalkWaves + w, lane r the active work column * 64 + r.  kPlace: the cells are written.
template <int kPlace>
__global__ __launch_bounds__(kWalkBlock) void k_lines_walk(LinesArgs a) {
  __shared__ uint32_t s_fig[5][kLinesChunkMax];          // works, whole, most, head, tail
  __shared__ uint32_t s_first[kLinesChunkMax];
  __shared__ unsigned long long s_sum[kLinesChunkMax];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t cg = blockIdx.x / a.n_chunks, ch = blockIdx.x % a.n_chunks;
  const uint32_t c = cg * kWalkWaves + wave;
  const uint32_t l_from = ch * a.chunk;
  const uint32_t nl = a.n_lines - l_from < a.chunk ? a.n_lines - l_from : a.chunk;
  for (uint32_t li = threadIdx.x; li < nl; li += kWalkBlock) {
#pragma unroll
    for (uint32_t f = 0; f < 5; ++f) s_fig[f][li] = 0;
    s_first[li] = FS_NONE;
    s_sum[li] = 0;
  }
  __syncthreads();
  if (c < a.n_cols) {                                    // (wave-uniform)
    const size_t ai = (size_t)c * 64 + lane;             // < stride: padding reads zeros
    const unsigned long long* cov = a.r.cov + ai;
    const uint32_t my_work = kPlace ? a.r.work_of[ai] : 0u;
    uint32_t w_lines = 0, w_whole = 0, w_cov = 0, w_words = 0;
    unsigned long long w_top = 0;
    // 64 lines at a time: a lane reads a line's incidence word and bounds, and the wave then
    // takes in turn the lines in which the column has a work (without the skip: all of them)
    for (uint32_t base = 0; base < nl; base += 64) {
      const uint32_t mine = base + lane;
      unsigned long long inc = 0;
      uint32_t lf_of = 0, le_of = 0;
      if (mine < nl) {
        inc = a.inc[(size_t)(l_from + mine) * a.n_cols + c];
        lf_of = a.line_first[l_from + mine];
        le_of = a.line_first[l_from + mine + 1] - 1;
      }
      uint64_t todo = __ballot(a.skip ? inc != 0 : mine < nl);
      while (todo) {
        const int from = __builtin_ctzll(todo);
        todo &= todo - 1;
        const uint32_t li = base + (uint32_t)from, l = l_from + li;
        const size_t at = (size_t)l * a.n_cols + c;
        const uint32_t lf = lane_u32(lf_of, (uint32_t)from), le = lane_u32(le_of, (uint32_t)from);
        const uint32_t k0 = lf >> 6, k1 = le >> 6;
        uint32_t covered = 0, first = 0, last = 0, runs = 0;
        unsigned long long carry = 0;
        for (uint32_t k = k0; k <= k1; ++k) {
          unsigned long long m = ~0ull;
          if (k == k0) m &= ~0ull << (lf & 63);
          if (k == k1) m &= ~0ull >> (63 - (le & 63));
          const unsigned long long x = cov[(size_t)k * a.stride] & m;
          if (x) {
            if (!covered) first = (k << 6) + (uint32_t)__builtin_ctzll(x);
            last = (k << 6) + 63 - (uint32_t)__builtin_clzll(x);
            covered += (uint32_t)__popcll(x);
            runs += (uint32_t)__popcll(x & ~((x << 1) | carry));
          }
          carry = x >> 63;
        }
        const bool cell = covered != 0;
        const uint64_t cells = __ballot(cell);
        if (!cells) continue;
        const uint32_t len = le - lf + 1;
        const bool whole = covered == len;
        const uint64_t b_whole = __ballot(whole);
        const uint64_t b_most = __ballot(
            cell && (unsigned long long)covered * 100ull >= (unsigned long long)a.most * len);
        const uint64_t b_head = __ballot(cell && first == lf);
        const uint64_t b_tail = __ballot(cell && last == le);
        const uint32_t sum = wave_sum(covered);
        if (lane == 0) {
          atomicAdd(&s_fig[0][li], (uint32_t)__popcll(cells));
          if (b_whole) atomicAdd(&s_fig[1][li], (uint32_t)__popcll(b_whole));
          if (b_most) atomicAdd(&s_fig[2][li], (uint32_t)__popcll(b_most));
          if (b_head) atomicAdd(&s_fig[3][li], (uint32_t)__popcll(b_head));
          if (b_tail) atomicAdd(&s_fig[4][li], (uint32_t)__popcll(b_tail));
          atomicAdd(&s_sum[li], (unsigned long long)sum);
          // the active numbers are in work order: the first set lane is the smallest work
          atomicMin(&s_first[li], a.r.work_of[(size_t)c * 64 + (uint32_t)__builtin_ctzll(cells)]);
        }
        if (cell) {
          ++w_lines;
          w_whole += whole;
          w_cov += covered;
          w_words += len;
          const unsigned long long key = ((unsigned long long)covered << 32) | (uint32_t)~l;
          if (key > w_top) w_top = key;
          if (kPlace) {
            const unsigned long long pos =
                a.off[l] + a.pre[at] + (uint32_t)__popcll(cells & ((1ull << lane) - 1));
            uint4* p = reinterpret_cast<uint4*>(a.cells + pos);
            p[0] = make_uint4(l, my_work, covered, first);
            p[1] = make_uint4(last, runs, 0u, 0u);
          }
        }
      }
    }
    // a work's sums leave once per chunk: 64 adjacent addresses per figure
    if (w_lines) {
      atomicAdd(&a.wacc[ai], w_lines);
      if (w_whole) atomicAdd(&a.wacc[a.stride + ai], w_whole);
      atomicAdd(&a.wacc[2 * a.stride + ai], w_cov);
      atomicAdd(&a.wacc[3 * a.stride + ai], w_words);
      atomicMax(&a.wtop[ai], w_top);
    }
  }
  __syncthreads();
  // a line's sums over the workgroup's columns: one atomic per figure that is not zero
  for (uint32_t li = threadIdx.x; li < nl; li += kWalkBlock) {
    if (!s_fig[0][li]) continue;
    fs_line* out = a.lines + (l_from + li);
    atomicAdd(&out->works, s_fig[0][li]);
    if (s_fig[1][li]) atomicAdd(&out->whole_works, s_fig[1][li]);
    if (s_fig[2][li]) atomicAdd(&out->most_works, s_fig[2][li]);
    if (s_fig[3][li]) atomicAdd(&out->head_works, s_fig[3][li]);
    if (s_fig[4][li]) atomicAdd(&out->tail_works, s_fig[4][li]);
    atomicMin(&out->first_work, s_first[li]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&out->covered_sum), s_sum[li]);
  }
}

// one lane per active work (each has a cell: its passages lie in lines)
__global__ __launch_bounds__(kRunBlock) void k_lines_works(LinesArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.r.n_active) return;
  const unsigned long long top = a.wtop[w];
  uint4* p = reinterpret_cast<uint4*>(a.works + w);
  p[0] = make_uint4(a.r.work_of[w], a.wacc[w], a.wacc[a.stride + w], a.wacc[2 * a.stride + w]);
  p[1] = make_uint4(a.wacc[3 * a.stride + w], ~(uint32_t)top, (uint32_t)(top >> 32), 0u);
}

// (fs_tiles.h's row popcounts are for its tiled matrix; named so that the unit compiles clean)
[[maybe_unused]] void (*const k_not_used)(CoverArgs) = k_pairs_covered;

thread_local double t_ms[3];    // tables, walk, total of the last call

// one call: tables() through the numbers of active works and cells, then walk()
struct LinesJob {
  CoverJob cj;
  DBuf<uint32_t> work_of, line_of, pre, cnt, wacc, bad;
  DBuf<unsigned long long> cov, inc, off, total, wtop;
  Clock<4> clk;
  LinesArgs a{};
  uint64_t n_cells = 0;
  uint32_t bad_lines = 0;

  int none(hipStream_t s) {
    if (a.n_lines)
      hipLaunchKernelGGL(k_lines_init, dim3(blocks_of(a.n_lines, kRunBlock)), dim3(kRunBlock), 0,
                         s, a.lines, a.n_lines);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }

  // a.r.n_active and n_cells set, the tables built (all on `s`, finished on return)
  int tables(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
             const uint32_t* d_line_first, uint32_t n_lines, uint32_t min_words, uint32_t max_gap,
             uint32_t most, fs_line* d_lines, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.r.n = n;
    a.r.n_works = n_works;
    a.r.n_script = n_script;
    a.r.nk = (n_script + 63) / 64;
    a.r.min_words = min_words;
    a.line_first = d_line_first;
    a.n_lines = n_lines;
    a.most = most;
    a.lines = d_lines;
    a.chunk = env_u32("FS_LINES_CHUNK", kLinesChunkDefault, kLinesChunkMax);
    if (!a.chunk) a.chunk = kLinesChunkDefault;
    a.skip = env_u32("FS_LINES_SKIP", 1u, 1u);
    if (!n || !n_lines) return none(s);
    // the line table's check and the word -> line map ride in front of number(), which waits
    // for the stream
    const dim3 blk(kRunBlock);
    FS_TRY(bad.reserve(1));
    FS_TRY(line_of.reserve(n_script));
    FS_HIP(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_lines_check, dim3(blocks_of((uint64_t)n_lines + 1, kRunBlock)), blk, 0,
                       s, d_line_first, n_lines, n_script, bad.p);
    if (n_script)
      hipLaunchKernelGGL(k_lines_map, dim3(blocks_of(n_script, kRunBlock)), blk, 0, s,
                         d_line_first, n_lines, n_script, line_of.p);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(&bad_lines, bad.p, sizeof bad_lines, hipMemcpyDeviceToHost, s));
    const int rc = cj.number(d_rows, a.r, max_gap, s);
    FS_HIP(hipStreamSynchronize(s));
    if (rc != FS_OK) return rc;
    if (bad_lines) {
      fs_set_error("line_first does not ascend strictly from 0 to n_script (%u) over %u lines",
                   n_script, n_lines);
      return FS_E_INVALID;
    }
    if (!a.r.n_active) return none(s);
    a.n_cols = a.r.n_tiles;                                  // kTile = 64 active works
    a.stride = (size_t)a.n_cols * 64;
    a.n_chunks = (n_lines + a.chunk - 1) / a.chunk;
    const uint64_t cov_words = (uint64_t)a.r.nk * a.stride;
    const uint64_t entries = (uint64_t)n_lines * a.n_cols;
    if (cov_words * 8 + entries * 12 > FS_LINES_MAX_BYTES) {
      fs_set_error("%u lines of %u script words over %u works with a passage: tables of more "
                   "than %u bytes", n_lines, n_script, a.r.n_active, FS_LINES_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    const uint64_t blocks = (uint64_t)((a.n_cols + kWalkWaves - 1) / kWalkWaves) * a.n_chunks;
    if (blocks > 0x7FFFFFFFull) {
      fs_set_error("%u lines over %u works with a passage: more chunks than a launch takes",
                   n_lines, a.r.n_active);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(work_of.reserve(a.stride));
    FS_TRY(cov.reserve((size_t)cov_words));
    FS_TRY(inc.reserve((size_t)entries));
    FS_TRY(pre.reserve((size_t)entries));
    FS_TRY(cnt.reserve(n_lines));
    FS_TRY(off.reserve(n_lines));
    FS_TRY(total.reserve(1));
    FS_TRY(wacc.reserve(4 * a.stride));
    FS_TRY(wtop.reserve(a.stride));
    FS_HIP(hipMemsetAsync(work_of.p, 0xFF, a.stride * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(cov.p, 0, (size_t)cov_words * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(inc.p, 0, (size_t)entries * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(wacc.p, 0, 4 * a.stride * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(wtop.p, 0, a.stride * sizeof(unsigned long long), s));
    a.r.work_of = work_of.p;
    a.r.cov = cov.p;
    a.line_of = line_of.p;
    a.inc = inc.p;
    a.pre = pre.p;
    a.cnt = cnt.p;
    a.off = off.p;
    a.total = total.p;
    a.wacc = wacc.p;
    a.wtop = wtop.p;
    FS_TRY(clk.mark(0, s));
    hipLaunchKernelGGL(k_pairs_list, dim3(blocks_of(n_works, kRunBlock)), blk, 0, s, a.r,
                       cj.flag.p);
    hipLaunchKernelGGL(k_lines_init, dim3(blocks_of(n_lines, kRunBlock)), blk, 0, s, d_lines,
                       n_lines);
    hipLaunchKernelGGL(k_lines_tables, dim3(blocks_of(a.r.n_runs, kRunBlock)), blk, 0, s,
                       RowsSrc{d_rows}, a, cj.flag.p);
    hipLaunchKernelGGL(k_lines_popc, dim3(blocks_of(n_lines, kRunBlock / 64)), blk, 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s, cnt.p,
                       (uint64_t)n_lines, off.p, total.p);
    FS_TRY(clk.mark(1, s));
    FS_HIP(hipGetLastError());
    unsigned long long tot = 0;
    FS_HIP(hipMemcpyAsync(&tot, total.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    n_cells = tot;
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[2] = t_ms[0];
    return FS_OK;
  }

  // the lines; with `place` the a.r.n_active works and the n_cells cells too (finished on
  // return)
  int walk(fs_line_work* d_works, fs_line_cell* d_cells, bool place, hipStream_t s) {
    if (!a.r.n_active) return FS_OK;                         // none() wrote the lines
    a.works = d_works;
    a.cells = d_cells;
    const uint32_t blocks = (a.n_cols + kWalkWaves - 1) / kWalkWaves * a.n_chunks;
    FS_TRY(clk.mark(2, s));
    if (place) {
      hipLaunchKernelGGL(k_lines_walk<1>, dim3(blocks), dim3(kWalkBlock), 0, s, a);
      hipLaunchKernelGGL(k_lines_works, dim3(blocks_of(a.r.n_active, kRunBlock)), dim3(kRunBlock),
                         0, s, a);
    } else {
      hipLaunchKernelGGL(k_lines_walk<0>, dim3(blocks), dim3(kWalkBlock), 0, s, a);
    }
    FS_TRY(clk.mark(3, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[1] = clk.elapsed(2, 3);
    t_ms[2] = t_ms[0] + t_ms[1];
    return FS_OK;
  }
};

// the rules both entry points share
int lines_check(uint64_t n_rows, uint32_t n_script, const void* line_first, uint32_t n_lines,
                uint32_t min_words, uint32_t most, const void* lines, const void* works,
                uint64_t works_cap, uint64_t* n_active, const void* cells, uint64_t cells_cap,
                uint64_t* n_cells) {
  if (!n_active || !n_cells || (n_lines && !lines) || (works_cap && !works) ||
      (cells_cap && !cells) || (n_rows && n_lines && !line_first)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (most < 1 || most > 100) {
    fs_set_error("most %u: a whole percentage, 1 to 100", most);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("lines", n_rows, n_script));
  *n_active = 0;
  *n_cells = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_lines(int device, const uint32_t* work, const uint32_t* fan_ix,
                        const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                        uint32_t n_script, const uint32_t* line_first, uint32_t n_lines,
                        uint32_t min_words, uint32_t max_gap, uint32_t most, fs_line* lines,
                        fs_line_work* works, uint64_t works_cap, uint64_t* n_active,
                        fs_line_cell* cells, uint64_t cells_cap, uint64_t* n_cells) {
  FS_TRY(lines_check(n_rows, n_script, line_first, n_lines, min_words, most, lines, works,
                     works_cap, n_active, cells, cells_cap, n_cells));
  if (!n_rows || !n_lines) {
    const fs_line none{0u, 0u, 0u, 0u, 0u, FS_NONE, 0u};
    for (uint32_t l = 0; l < n_lines; ++l) lines[l] = none;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_line_first;
  DBuf<fs_line> d_lines;
  DBuf<fs_line_work> d_works;
  DBuf<fs_line_cell> d_cells;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_line_first.upload(line_first, (size_t)n_lines + 1, nullptr));
  FS_TRY(d_lines.reserve(n_lines));
  LinesJob job;
  FS_TRY(job.tables(rows.p, n, n_works, n_script, d_line_first.p, n_lines, min_words, max_gap, most,
                    d_lines.p, nullptr));
  *n_active = job.a.r.n_active;
  *n_cells = job.n_cells;
  const bool place = job.a.r.n_active <= works_cap && job.n_cells <= cells_cap;
  if (place) {
    FS_TRY(d_works.reserve(job.a.r.n_active));
    FS_TRY(d_cells.reserve(job.n_cells));
  }
  FS_TRY(job.walk(d_works.p, d_cells.p, place, nullptr));
  FS_TRY(copy_out(lines, d_lines, n_lines));
  if (!place) return FS_E_CAPACITY;
  if (job.a.r.n_active) FS_TRY(copy_out(works, d_works, job.a.r.n_active));
  if (job.n_cells) FS_TRY(copy_out(cells, d_cells, job.n_cells));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_lines_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                             uint32_t n_works, const uint32_t* d_line_first, uint32_t n_lines,
                             uint32_t min_words, uint32_t max_gap, uint32_t most,
                             fs_line* d_lines, fs_line_work* d_works, uint64_t works_cap,
                             uint64_t* n_active, fs_line_cell* d_cells, uint64_t cells_cap,
                             uint64_t* n_cells) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: lines take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(lines_check(n_rows, (uint32_t)ix->n_script, d_line_first, n_lines, min_words, most,
                     d_lines, d_works, works_cap, n_active, d_cells, cells_cap, n_cells));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_line_first & 3) ||
      ((uintptr_t)d_lines & 15) || ((uintptr_t)d_works & 15) || ((uintptr_t)d_cells & 15)) {
    fs_set_error("d_rows, d_lines, d_works and d_cells must be 16-byte aligned device pointers, "
                 "d_line_first 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  LinesJob job;
  FS_TRY(job.tables(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_line_first,
                    n_lines, min_words, max_gap, most, d_lines, ix->stream));
  *n_active = job.a.r.n_active;
  *n_cells = job.n_cells;
  const bool place = job.a.r.n_active <= works_cap && job.n_cells <= cells_cap;
  FS_TRY(job.walk(d_works, d_cells, place, ix->stream));
  return place ? FS_OK : FS_E_CAPACITY;
}

extern "C" int fs_lines_times(double* ms) {
  return times_out(ms, t_ms, 3);
}
