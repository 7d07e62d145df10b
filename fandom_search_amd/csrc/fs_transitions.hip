// fs_transitions.hip -- `ao3.py transitions`: which stretch of the script the fan works quote
// next (fs_transitions, fs_transitions_rows in include/fandom_search.h).  The passages of
// fs_passages that start in a unit (a quoted region, a scene, a character) are a work's
// sequence; two neighbours of it close enough in the fan work are a step from unit a to unit b,
// and cell (a, b) counts its steps, those that advance in the script, its distinct works and
// the smallest of them.  The product is tiny and contention is everything: a corpus under
// `--by character` sends a million steps into a few hundred cells.
//
// Why no schedule changes the result: every value is an integer; adds and minima commute; a
// distinct count is a set (fs_probe.h) whose membership does not depend on who inserted, and
// the one call that inserts a key adds one; best_next is the maximum of a single 64-bit key
// (steps << 32 | ~b), which holds the tie rule; and the cells' places come from scanned counts
// and from counting the cells in front, never from arrival.
//
// Separate launches; no workgroup waits on another (the first four are fs_sequence.h, which
// fs_routes.hip shares):
//   k_tr_check     one lane per record: work < n_works, orig_ix < n_script
//   k_tr_units_ok  one lane per script word: a unit number that is neither < n_units nor none
//   (fs_runs_find) the run heads, as fs_passages joins them
//   k_tr_seq       one lane per run: kept runs that start in a unit counted per workgroup, then
//                  (after k_tr_scan) placed in record order as columns
//   k_tr_count     one lane per sequence element: it looks at the element before (a change of
//                  work: a start) and behind (a change of work: an end; else, within reach, a
//                  step).  Two classes by n_units:
//                    dense   (n_units <= FS_TRANSITIONS_DENSE) cell (a, b) is index a * n_units
//                            + b; a workgroup keeps every per-cell and per-unit figure in LDS
//                            (LDS atomic add and max) over all the elements it strides through
//                            and then adds its non-zero entries to the global arrays, one
//                            atomic each: no global atomic per step goes to a counter
//                    hashed  the cell is the slot of a << 32 | b in a table, its counters beside
//                            the slot; every figure is a global atomic
//                  Distinct works are set inserts of (cell, work) and (unit, work) in both.
//   k_tr_keep      one lane per cell index: the keep rule, successors, predecessors, best_next
//   k_tr_scan      one workgroup: a unit's first kept cell
//   k_tr_units     one lane per unit: its fs_transition_unit
//   k_tr_scatter   one lane per cell index: a kept cell to a free place of its unit's range
//   k_tr_rank      one lane per kept cell: the cells of its unit with a smaller b are its place;
//                  a unit of more than kLong kept cells is counted by the whole wave
#include "fs_probe.h"
#include "fs_sequence.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kDenseMax = 64;          // units of the dense class at most
constexpr uint32_t kDenseGroups = 1024;     // workgroups of its counting pass at most
constexpr uint32_t kLong = 64;              // units of more kept cells are ranked by a wave

static_assert(sizeof(fs_transition_unit) == 40 && sizeof(fs_transition) == 32, "fs_transitions");

// per-unit figures counted by k_tr_count, [figure][unit]
enum { kUPassages = 0, kUWorks, kUStarts, kUEnds, kUOut, kUIn, kUFigures };
// per-cell figures; the smallest work is kept as the largest ~work, 0 for none
enum { kCSteps = 0, kCAdvances, kCWorks, kCFirst, kCFigures };

struct TrArgs : SeqArgs {        // the records and the sequence: fs_sequence.h
  uint32_t within, min_steps, min_step_works, min_share;
  uint64_t mask;                 // slots - 1 of each table
  uint64_t hash_mask;            // FS_TRANSITIONS_HASH_BITS: the bits of a key's hash kept
  uint64_t n_index;              // cell indices: n_units^2 (dense) or slots (hashed)
  unsigned long long* cell_tab;  // hashed: a << 32 | b
  unsigned long long* cw_tab;    // cell index << 32 | work
  unsigned long long* uw_tab;    // unit << 32 | work
  uint4* cell_cnt;               // [n_index] {steps, advances, works, ~first_work}
  uint32_t* ufig;                // [kUFigures][n_units]
  uint32_t* succ;                // [n_units] each: kept cells (u, .), kept cells (., u),
  uint32_t* pred;                //   the first place of the unit's kept cells, those placed
  uint32_t* first;
  uint32_t* cursor;
  unsigned long long* best;      // [n_units] steps << 32 | ~b of the best kept cell
  unsigned long long* total;     // kept cells
  fs_transition_unit* units;
  fs_transition* tmp;            // the kept cells, unit by unit, unranked
  fs_transition* cells;
};

// the slot of `key` in `tab`; true when this call put it there
__device__ inline bool set_insert(const TrArgs& a, unsigned long long* tab, unsigned long long key,
                                  uint64_t* slot) {
  bool inserted;
  *slot = fs_probe_insert(tab, a.mask, fs_mix64(fs_mix64(key) & a.hash_mask), key,
                          [key](unsigned long long cur) { return cur == key; }, &inserted);
  return inserted;
}

// One lane per sequence element, the workgroup striding through the sequence.  kDense: the
// figures in LDS until the end, where each non-zero one is a single global atomic.
template <bool kDense>
__global__ __launch_bounds__(kBlock) void k_tr_count(TrArgs a) {
  __shared__ uint32_t s_cell[kDense ? kCFigures * kDenseMax * kDenseMax : 1];
  __shared__ uint32_t s_unit[kDense ? kUFigures * kDenseMax : 1];
  const uint32_t nu = a.n_units;
  const uint32_t nc = kDense ? nu * nu : 0u;
  if (kDense) {
    for (uint32_t i = threadIdx.x; i < kCFigures * nc; i += kBlock) s_cell[i] = 0u;
    for (uint32_t i = threadIdx.x; i < kUFigures * nu; i += kBlock) s_unit[i] = 0u;
    __syncthreads();
  }
  uint32_t* cell_words = reinterpret_cast<uint32_t*>(a.cell_cnt);
  const auto unit_add = [&](uint32_t figure, uint32_t u) {
    if (kDense) atomicAdd(&s_unit[figure * nu + u], 1u);
    else atomicAdd(&a.ufig[(size_t)figure * nu + u], 1u);
  };
  const auto cell_add = [&](uint32_t figure, uint64_t c) {
    if (kDense) atomicAdd(&s_cell[figure * nc + (uint32_t)c], 1u);
    else atomicAdd(&cell_words[c * kCFigures + figure], 1u);
  };
  for (uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x; p < a.n_seq;
       p += (uint64_t)gridDim.x * kBlock) {
    const uint32_t w = a.work[p], u = a.unit[p];
    const bool start = p == 0 || a.work[p - 1] != w;
    const bool more = p + 1 < a.n_seq && a.work[p + 1] == w;
    uint64_t slot;
    unit_add(kUPassages, u);
    if (start) unit_add(kUStarts, u);
    if (!more) unit_add(kUEnds, u);
    if (set_insert(a, a.uw_tab, (unsigned long long)u << 32 | w, &slot)) unit_add(kUWorks, u);
    if (!more) continue;
    if (a.within != FS_NONE && (int64_t)a.ff[p + 1] - (int64_t)a.fl[p] > (int64_t)a.within + 1)
      continue;
    const uint32_t b = a.unit[p + 1];
    uint64_t c = (uint64_t)u * nu + b;
    if (!kDense) set_insert(a, a.cell_tab, (unsigned long long)u << 32 | b, &c);
    unit_add(kUOut, u);
    unit_add(kUIn, b);
    cell_add(kCSteps, c);
    if (a.of[p + 1] > a.ol[p]) cell_add(kCAdvances, c);
    if (set_insert(a, a.cw_tab, (unsigned long long)c << 32 | w, &slot)) cell_add(kCWorks, c);
    if (kDense) atomicMax(&s_cell[kCFirst * nc + (uint32_t)c], ~w);
    else atomicMax(&cell_words[c * kCFigures + kCFirst], ~w);
  }
  if (!kDense) return;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < kCFigures * nc; i += kBlock) {
    const uint32_t v = s_cell[i], figure = i / nc, c = i % nc;
    if (!v) continue;
    if (figure == kCFirst) atomicMax(&cell_words[(size_t)c * kCFigures + figure], v);
    else atomicAdd(&cell_words[(size_t)c * kCFigures + figure], v);
  }
  for (uint32_t i = threadIdx.x; i < kUFigures * nu; i += kBlock)
    if (s_unit[i]) atomicAdd(&a.ufig[i], s_unit[i]);
}

// cell index i: false when it holds no kept cell, else the cell
template <bool kDense>
__device__ inline bool kept_cell(const TrArgs& a, uint64_t i, fs_transition* c) {
  uint32_t from, to;
  if (kDense) {
    from = (uint32_t)(i / a.n_units);
    to = (uint32_t)(i % a.n_units);
  } else {
    const unsigned long long key = a.cell_tab[i];
    if (key == kProbeEmpty) return false;
    from = (uint32_t)(key >> 32);
    to = (uint32_t)key;
  }
  const uint4 n = a.cell_cnt[i];
  const uint32_t out = a.ufig[(size_t)kUOut * a.n_units + from];
  if (n.x < a.min_steps || n.z < a.min_step_works ||
      (unsigned long long)n.x * 100ull < (unsigned long long)a.min_share * out)
    return false;
  *c = fs_transition{from, to, n.x, n.y, n.z, ~n.w, out, a.ufig[(size_t)kUIn * a.n_units + to]};
  return true;
}

template <bool kDense>
__global__ __launch_bounds__(kBlock) void k_tr_keep(TrArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  fs_transition c;
  if (i >= a.n_index || !kept_cell<kDense>(a, i, &c)) return;
  atomicAdd(&a.succ[c.a], 1u);
  atomicAdd(&a.pred[c.b], 1u);
  atomicMax(&a.best[c.a], (unsigned long long)c.steps << 32 | (uint32_t)~c.b);
}

__global__ __launch_bounds__(kBlock) void k_tr_units(TrArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u >= a.n_units) return;
  const size_t nu = a.n_units;
  const unsigned long long key = a.best[u];
  a.units[u] = fs_transition_unit{a.ufig[kUPassages * nu + u], a.ufig[kUWorks * nu + u],
                                  a.ufig[kUStarts * nu + u],   a.ufig[kUEnds * nu + u],
                                  a.ufig[kUOut * nu + u],      a.ufig[kUIn * nu + u],
                                  a.succ[u],                   a.pred[u],
                                  key ? ~(uint32_t)key : FS_NONE, (uint32_t)(key >> 32)};
}

// a unit nobody quotes (no records, no units' worth of passages)
__global__ __launch_bounds__(kBlock) void k_tr_units_none(fs_transition_unit* units,
                                                          uint32_t n_units) {
  const uint64_t u = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u < n_units) units[u] = fs_transition_unit{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, FS_NONE, 0u};
}

template <bool kDense>
__global__ __launch_bounds__(kBlock) void k_tr_scatter(TrArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  fs_transition c;
  if (i >= a.n_index || !kept_cell<kDense>(a, i, &c)) return;
  a.tmp[a.first[c.a] + atomicAdd(&a.cursor[c.a], 1u)] = c;
}

__global__ __launch_bounds__(kBlock) void k_tr_rank(TrArgs a, uint32_t n_cells) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool live = p < n_cells;
  fs_transition c{};
  uint32_t first = 0, len = 0, rank = 0;
  if (live) {
    c = a.tmp[p];
    first = a.first[c.a];
    len = a.succ[c.a];
  }
  const bool is_long = live && len > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)first, j);
    const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)len, j);
    const uint32_t bj = (uint32_t)__builtin_amdgcn_readlane((int)c.b, j);
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) before += a.tmp[fj + k].b < bj ? 1u : 0u;
    before = wave_sum(before);
    if ((int)lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k) rank += a.tmp[first + k].b < c.b ? 1u : 0u;
  if (live) a.cells[first + rank] = c;
}

thread_local double t_ms[5];    // sequence, count, keep, place, total of the last call

uint64_t tr_hash_mask() {
  const char* e = getenv("FS_TRANSITIONS_HASH_BITS");   // diagnostic: k bits of a hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  if (k <= 0) return 0ull;
  return k >= 64 ? ~0ull : (1ull << k) - 1;
}

// one call: count() through the per-unit results and the number of kept cells, then write()
struct TrJob {
  SeqJob sq;
  DBuf<uint32_t> ufig;
  DBuf<unsigned long long> cell_tab, cw_tab, uw_tab, best, total;
  DBuf<uint4> cell_cnt;
  DBuf<fs_transition> tmp;
  Clock<6> clk;
  TrArgs a{};
  bool dense = false;
  uint64_t n_cells = 0;

  int none(hipStream_t s) {
    if (a.n_units)
      hipLaunchKernelGGL(k_tr_units_none, dim3(blocks_of(a.n_units, kBlock)), dim3(kBlock), 0, s,
                         a.units, a.n_units);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }

  // d_units written, n_cells set (all on `s`, finished on return)
  int count(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
            const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
            uint32_t within, uint32_t min_steps, uint32_t min_step_works, uint32_t min_share,
            fs_transition_unit* d_units, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.unit_of = d_unit_of;
    a.n_units = n_units;
    a.min_words = min_words;
    a.within = within;
    a.min_steps = min_steps;
    a.min_step_works = min_step_works;
    a.min_share = min_share;
    a.units = d_units;
    if (!n || !n_units) return none(s);
    const dim3 blk(kBlock);
    FS_TRY(clk.mark(0, s));
    FS_TRY(sq.list(d_rows, a, max_gap, s));
    if (!a.n_seq) return none(s);
    const size_t m = a.n_seq, nu = n_units;
    FS_TRY(clk.mark(1, s));

    // the figures.  FS_TRANSITIONS_DENSE: a diagnostic, read on each call
    dense = n_units <= env_u32("FS_TRANSITIONS_DENSE", kDenseMax, kDenseMax);
    uint64_t slots = fs_probe_slots(m);
    if (slots > (1ull << 32)) slots = 1ull << 32;            // (a cell's slot number is 32 bits)
    a.mask = slots - 1;
    a.hash_mask = tr_hash_mask();
    a.n_index = dense ? (uint64_t)n_units * n_units : slots;
    FS_TRY(cw_tab.reserve(slots));
    FS_TRY(uw_tab.reserve(slots));
    if (!dense) FS_TRY(cell_tab.reserve(slots));
    FS_TRY(cell_cnt.reserve(a.n_index));
    FS_TRY(ufig.reserve((kUFigures + 4) * nu));
    FS_TRY(best.reserve(nu));
    FS_TRY(total.reserve(1));
    FS_HIP(hipMemsetAsync(cw_tab.p, 0xFF, slots * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(uw_tab.p, 0xFF, slots * sizeof(unsigned long long), s));
    if (!dense) FS_HIP(hipMemsetAsync(cell_tab.p, 0xFF, slots * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(cell_cnt.p, 0, a.n_index * sizeof(uint4), s));
    FS_HIP(hipMemsetAsync(ufig.p, 0, (kUFigures + 4) * nu * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(best.p, 0, nu * sizeof(unsigned long long), s));
    a.cell_tab = cell_tab.p;
    a.cw_tab = cw_tab.p;
    a.uw_tab = uw_tab.p;
    a.cell_cnt = cell_cnt.p;
    a.ufig = ufig.p;
    a.succ = ufig.p + kUFigures * nu;
    a.pred = a.succ + nu;
    a.first = a.pred + nu;
    a.cursor = a.first + nu;
    a.best = best.p;
    a.total = total.p;
    const uint32_t seq_blocks = blocks_of(m, kBlock);
    const uint32_t index_blocks = blocks_of(a.n_index, kBlock);
    if (dense)
      hipLaunchKernelGGL(k_tr_count<true>,
                         dim3(seq_blocks < kDenseGroups ? seq_blocks : kDenseGroups), blk, 0, s, a);
    else
      hipLaunchKernelGGL(k_tr_count<false>, dim3(seq_blocks), blk, 0, s, a);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(2, s));
    if (dense) hipLaunchKernelGGL(k_tr_keep<true>, dim3(index_blocks), blk, 0, s, a);
    else hipLaunchKernelGGL(k_tr_keep<false>, dim3(index_blocks), blk, 0, s, a);
    hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(kScanBlock), 0, s, a.succ, a.first, n_units,
                       a.total, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_tr_units, dim3(blocks_of(n_units, kBlock)), blk, 0, s, a);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(3, s));
    unsigned long long tot = 0;
    FS_HIP(hipMemcpyAsync(&tot, total.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    n_cells = tot;
    for (int j = 0; j < 3; ++j) t_ms[j] = clk.elapsed(j, j + 1);
    t_ms[4] = clk.elapsed(0, 3);
    return FS_OK;
  }

  // the n_cells kept cells into d_cells (finished on return)
  int write(fs_transition* d_cells, hipStream_t s) {
    if (!n_cells) return FS_OK;
    FS_TRY(tmp.reserve(n_cells));
    a.tmp = tmp.p;
    a.cells = d_cells;
    const dim3 blk(kBlock), index_grid(blocks_of(a.n_index, kBlock));
    FS_TRY(clk.mark(4, s));
    if (dense) hipLaunchKernelGGL(k_tr_scatter<true>, index_grid, blk, 0, s, a);
    else hipLaunchKernelGGL(k_tr_scatter<false>, index_grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_tr_rank, dim3(blocks_of(n_cells, kBlock)), blk, 0, s, a,
                       (uint32_t)n_cells);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(5, s));
    FS_HIP(hipStreamSynchronize(s));
    t_ms[3] = clk.elapsed(4, 5);
    t_ms[4] += t_ms[3];
    return FS_OK;
  }
};

// the rules both entry points share
int tr_check(uint64_t n_rows, uint32_t n_script, const void* unit_of, uint32_t n_units,
             uint32_t min_words, uint32_t min_steps, uint32_t min_step_works, uint32_t min_share,
             const void* units, const void* cells, uint64_t cap, uint64_t* n_cells) {
  if (!n_cells || (n_units && !units) || (cap && !cells) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_steps == 0 || min_step_works == 0) {
    fs_set_error("min_words, min_steps and min_step_works must be at least 1");
    return FS_E_INVALID;
  }
  if (min_share > 100) {
    fs_set_error("min_share %u: a whole percentage, 0 to 100", min_share);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("transitions", n_rows, n_script));
  *n_cells = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_transitions(int device, const uint32_t* work, const uint32_t* fan_ix,
                              const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                              uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                              uint32_t min_words, uint32_t max_gap, uint32_t within,
                              uint32_t min_steps, uint32_t min_step_works, uint32_t min_share,
                              fs_transition_unit* units, fs_transition* cells, uint64_t cap,
                              uint64_t* n_cells) {
  FS_TRY(tr_check(n_rows, n_script, unit_of, n_units, min_words, min_steps, min_step_works,
                  min_share, units, cells, cap, n_cells));
  if (!n_rows || !n_units) {
    const fs_transition_unit none{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, FS_NONE, 0u};
    for (uint32_t u = 0; u < n_units; ++u) units[u] = none;
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
  DBuf<uint32_t> d_unit_of;
  DBuf<fs_transition_unit> d_units;
  DBuf<fs_transition> d_cells;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n_script, nullptr));
  FS_TRY(d_units.reserve(n_units));
  TrJob job;
  FS_TRY(job.count(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap, within,
                   min_steps, min_step_works, min_share, d_units.p, nullptr));
  FS_TRY(copy_out(units, d_units, n_units));
  *n_cells = job.n_cells;
  if (job.n_cells > cap) {
    fs_set_error("%llu cells need room", (unsigned long long)job.n_cells);
    return FS_E_CAPACITY;
  }
  if (job.n_cells) {
    FS_TRY(d_cells.reserve(job.n_cells));
    FS_TRY(job.write(d_cells.p, nullptr));
    FS_TRY(copy_out(cells, d_cells, job.n_cells));
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_transitions_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                   uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                                   uint32_t min_words, uint32_t max_gap, uint32_t within,
                                   uint32_t min_steps, uint32_t min_step_works,
                                   uint32_t min_share, fs_transition_unit* d_units,
                                   fs_transition* d_cells, uint64_t cap, uint64_t* n_cells) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: transitions take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(tr_check(n_rows, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, min_steps,
                  min_step_works, min_share, d_units, d_cells, cap, n_cells));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 3) || ((uintptr_t)d_cells & 3)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_unit_of, d_units and "
                 "d_cells 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  TrJob job;
  FS_TRY(job.count(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                   min_words, max_gap, within, min_steps, min_step_works, min_share, d_units,
                   ix->stream));
  *n_cells = job.n_cells;
  if (job.n_cells > cap) {
    fs_set_error("%llu cells need room", (unsigned long long)job.n_cells);
    return FS_E_CAPACITY;
  }
  return job.write(d_cells, ix->stream);
}

extern "C" int fs_transitions_times(double* ms) {
  return times_out(ms, t_ms, 5);
}
