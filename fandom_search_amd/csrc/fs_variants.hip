// fs_variants.hip -- `ao3.py variants`: records (work, orig_ix, spell) in any order grouped by
// script word and spelling (fs_variants in include/fandom_search.h): per (script word,
// spelling) cell its records and distinct works, per script word its records, spellings and
// works, the cells ranked inside their word.
//
// Every output is a count or a distinct count, so nothing is sorted on the way in.  The three
// distinct counts are one set primitive (fs_probe.h: an open-addressing table of 64-bit keys;
// the call that inserts a key adds one, as fs_works does with the bits atomicOr finds clear)
// over three integer keys: (orig_ix, spell) gives the cells, (cell, work) a cell's works,
// (orig_ix, work) a word's works.  Separate launches; no workgroup waits on another:
//   k_var_insert   one lane per record: the three inserts and the counters behind them
//   k_var_scan     one workgroup over the script: cells per word scanned, a word's first cell
//   k_var_scatter  one lane per slot of the cell table: a cell to a free place of its word
//   k_var_rank     one lane per cell: the cells of its word that precede it are its place; a
//                  word of more than kLong cells is counted by the whole wave
#include "fs_internal.h"
#include "fs_probe.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kScanItems = 4;          // script words per thread of the one-workgroup scan
constexpr uint32_t kLong = 64;              // words of more cells than this are ranked by a wave

static_assert(sizeof(fs_variant_cell) == 16 && sizeof(fs_variant_word) == 16, "fs_variants");
static_assert(offsetof(fs_variant_word, n_records) == 0 && offsetof(fs_variant_word, n_spellings) == 4 &&
              offsetof(fs_variant_word, n_works) == 8, "fs_variant_word");

struct VarArgs {
  const uint32_t* work;
  const uint32_t* orig;
  const uint32_t* spell;
  uint32_t n, n_works, n_script, n_spell, n_cells;
  uint64_t mask;                 // slots - 1 of each of the three tables
  unsigned long long* cell_tab;  // orig_ix << 32 | spell
  unsigned long long* cw_tab;    // cell slot << 32 | work
  unsigned long long* ow_tab;    // orig_ix << 32 | work
  uint2* cell_cnt;               // [slots] {records, works} of the cell in that slot
  uint32_t* cursor;              // [n_script] cells of a word placed so far
  uint32_t* status;              // [0] invalid input, [1] cells
  fs_variant_word* words;
  fs_variant_cell* tmp;          // the cells, word by word, unranked
  fs_variant_cell* cells;
};

// the slot of `key` in `tab`; true when this call put it there
__device__ inline bool set_insert(unsigned long long* tab, uint64_t mask, unsigned long long key,
                                  uint64_t* slot) {
  bool inserted;
  *slot = fs_probe_insert(tab, mask, fs_mix64(key), key,
                          [key](unsigned long long cur) { return cur == key; }, &inserted);
  return inserted;
}

__global__ __launch_bounds__(kBlock) void k_var_insert(VarArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool bad = false;
  if (i < a.n) {
    const uint32_t w = a.work[i], o = a.orig[i], s = a.spell[i];
    bad = w >= a.n_works || o >= a.n_script || s >= a.n_spell;
    if (!bad) {
      uint32_t* __restrict__ wc = reinterpret_cast<uint32_t*>(a.words + o);
      uint64_t cell, other;
      atomicAdd(&wc[0], 1u);
      if (set_insert(a.cell_tab, a.mask, (unsigned long long)o << 32 | s, &cell)) atomicAdd(&wc[1], 1u);
      atomicAdd(&a.cell_cnt[cell].x, 1u);
      if (set_insert(a.cw_tab, a.mask, (unsigned long long)cell << 32 | w, &other))
        atomicAdd(&a.cell_cnt[cell].y, 1u);
      if (set_insert(a.ow_tab, a.mask, (unsigned long long)o << 32 | w, &other)) atomicAdd(&wc[2], 1u);
    }
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 1u);
}

// One workgroup over the script, chunks of 4096 words in turn: first_cell = the cells of the
// words in front (0xFFFFFFFF for a word without any); status[1] = cells.
__global__ __launch_bounds__(kScanBlock) void k_var_scan(VarArgs a) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  const uint32_t cells = scan_chunks<kScanItems, uint32_t, uint32_t>(
      a.n_script, [&a](uint64_t j) { return a.words[j].n_spellings; },
      [&a](uint64_t j, uint32_t at, uint32_t x) { a.words[j].first_cell = x ? at : FS_NONE; }, s_w);
  if (threadIdx.x == 0) a.status[1] = cells;
}

__global__ __launch_bounds__(kBlock) void k_var_scatter(VarArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const unsigned long long key = a.cell_tab[slot];
  if (key == kProbeEmpty) return;
  const uint32_t o = (uint32_t)(key >> 32);
  const uint2 c = a.cell_cnt[slot];
  a.tmp[a.words[o].first_cell + atomicAdd(&a.cursor[o], 1u)] =
      fs_variant_cell{o, (uint32_t)key, c.x, c.y};
}

// x stands in front of y inside their word
__device__ inline bool precedes(const fs_variant_cell& x, const fs_variant_cell& y) {
  if (x.n_records != y.n_records) return x.n_records > y.n_records;
  if (x.n_works != y.n_works) return x.n_works > y.n_works;
  return x.spell < y.spell;
}

__global__ __launch_bounds__(kBlock) void k_var_rank(VarArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool live = p < a.n_cells;
  fs_variant_cell c{};
  uint32_t first = 0, len = 0, rank = 0;
  if (live) {
    c = a.tmp[p];
    first = a.words[c.orig_ix].first_cell;
    len = a.words[c.orig_ix].n_spellings;
  }
  const bool is_long = live && len > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)first, j);
    const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)len, j);
    fs_variant_cell cj;
    cj.orig_ix = fj;                                           // (not compared)
    cj.spell = (uint32_t)__builtin_amdgcn_readlane((int)c.spell, j);
    cj.n_records = (uint32_t)__builtin_amdgcn_readlane((int)c.n_records, j);
    cj.n_works = (uint32_t)__builtin_amdgcn_readlane((int)c.n_works, j);
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) before += precedes(a.tmp[fj + k], cj) ? 1u : 0u;
    before = wave_sum(before);
    if ((int)lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k) rank += precedes(a.tmp[first + k], c) ? 1u : 0u;
  if (live) a.cells[first + rank] = c;
}

int variants_invalid() {
  fs_set_error("a work >= n_works, an orig_ix >= n_script or a spell >= n_spell");
  return FS_E_INVALID;
}

}  // namespace

extern "C" int fs_variants(int device, const uint32_t* work, const uint32_t* orig_ix,
                           const uint32_t* spell, uint64_t n, uint32_t n_works, uint32_t n_script,
                           uint32_t n_spell, fs_variant_word* words, fs_variant_cell* cells,
                           uint64_t cap, uint64_t* n_cells) {
  if (!n_cells || (n_script && !words) || (cap && !cells)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("variants", n, n_script));
  *n_cells = 0;
  if (n == 0) {
    for (uint32_t j = 0; j < n_script; ++j) words[j] = fs_variant_word{0, 0, 0, FS_NONE};
    return FS_OK;
  }
  if (!work || !orig_ix || !spell) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (!n_works || !n_script || !n_spell) return variants_invalid();
  FS_ENTER(device);
  uint64_t slots = fs_probe_slots(n);
  if (slots > (1ull << 32)) slots = 1ull << 32;              // (a cell's slot number is 32 bits)
  DBuf<uint32_t> d_work, d_orig, d_spell, d_cursor, d_status;
  DBuf<unsigned long long> d_cell, d_cw, d_ow;
  DBuf<uint2> d_cnt;
  DBuf<fs_variant_word> d_words;
  DBuf<fs_variant_cell> d_tmp, d_cells;
  FS_TRY(d_work.upload(work, n, nullptr));
  FS_TRY(d_orig.upload(orig_ix, n, nullptr));
  FS_TRY(d_spell.upload(spell, n, nullptr));
  FS_TRY(d_cell.reserve(slots));
  FS_TRY(d_cw.reserve(slots));
  FS_TRY(d_ow.reserve(slots));
  FS_TRY(d_cnt.reserve(slots));
  FS_TRY(d_cursor.reserve(n_script));
  FS_TRY(d_status.reserve(4));
  FS_TRY(d_words.reserve(n_script));
  FS_HIP(hipMemsetAsync(d_cell.p, 0xFF, slots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_cw.p, 0xFF, slots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_ow.p, 0xFF, slots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_cnt.p, 0, slots * sizeof(uint2), nullptr));
  FS_HIP(hipMemsetAsync(d_cursor.p, 0, (size_t)n_script * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_status.p, 0, 4 * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_words.p, 0, (size_t)n_script * sizeof(fs_variant_word), nullptr));
  VarArgs a{};
  a.work = d_work.p;
  a.orig = d_orig.p;
  a.spell = d_spell.p;
  a.n = (uint32_t)n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.n_spell = n_spell;
  a.mask = slots - 1;
  a.cell_tab = d_cell.p;
  a.cw_tab = d_cw.p;
  a.ow_tab = d_ow.p;
  a.cell_cnt = d_cnt.p;
  a.cursor = d_cursor.p;
  a.status = d_status.p;
  a.words = d_words.p;
  hipLaunchKernelGGL(k_var_insert, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_var_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  uint32_t st[2];
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) return variants_invalid();
  *n_cells = st[1];
  FS_TRY(copy_out(words, d_words, n_script));
  if (st[1] > cap) {
    fs_set_error("%u cells need room", st[1]);
    return FS_E_CAPACITY;
  }
  a.n_cells = st[1];
  FS_TRY(d_tmp.reserve(a.n_cells));
  FS_TRY(d_cells.reserve(a.n_cells));
  a.tmp = d_tmp.p;
  a.cells = d_cells.p;
  hipLaunchKernelGGL(k_var_scatter, dim3((uint32_t)((slots + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, nullptr, a);
  hipLaunchKernelGGL(k_var_rank, dim3((a.n_cells + kBlock - 1) / kBlock), dim3(kBlock), 0, nullptr,
                     a);
  FS_HIP(hipGetLastError());
  FS_TRY(copy_out(cells, d_cells, a.n_cells));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}
