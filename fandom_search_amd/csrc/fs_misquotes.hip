// fs_misquotes.hip -- `ao3.py misquotes`: the works that share departures from the script
// (fs_misquotes in include/fandom_search.h).  The matrix is works x (script word, wrong
// spelling): hundreds of thousands of columns and a handful of bits per row, so the product of
// a work with a work is sparse: a posting list per telling misquote, every list expanded into
// its pairs of works, and a hash table that accumulates per pair.
//
// Nothing is sorted globally and every figure is an integer sum, minimum or maximum, so no
// schedule changes a result.  The sets are the set primitive of fs_variants (fs_probe.h);
// FS_MISQUOTES_HASH_BITS cuts every table's hash down to prove the hash decides nothing.
// Separate launches; no workgroup waits on another:
//   k_mq_check / k_mq_same   records and same[] in range; (fs_runs_find) the run heads
//   k_mq_cells      one lane per record: its run by a binary search in the heads; inside a kept
//                   run the inserts of (o, work), (o, spell), (cell, work) and their counters
//   k_mq_classify   one lane per cell slot: listed or not; the listed cells per word
//   k_mq_scatter / k_mq_number   the listed cells to their word, ranked there: the misquotes,
//                   telling or not, with their weight
//   k_mq_count      one lane per (cell, work): per work its listed, telling and singular
//   k_mq_offsets    one workgroup: list offsets, contribution offsets (64 bits), work offsets
//   k_mq_post / k_mq_rank   both postings scattered, then ranked inside their list (a list of
//                   more than kLong entries by the whole wave)
//   k_mq_expand     the hot path: one lane per contribution t < P, whatever list it is of: the
//                   list by a binary search in the contribution offsets, the pair by unranking
//                   the triangle, one insert and three atomics
//   k_mq_keep / k_mq_rows / k_mq_rank / k_mq_row_bits   the keep rule per slot, partners,
//                   closest; the kept pairs counted per a, scattered and ranked by b (a row of
//                   more than kLong partners by a bit per work in LDS)
//   k_mq_finish     the works table
//   k_mq_detail     one lane per kept pair: both telling lists walked against the readers set
#include "fs_internal.h"
#include "fs_probe.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kLong = 64;              // lists of more entries than this are ranked by a wave
constexpr uint64_t kMaxRows = 1ull << 27;
constexpr size_t kRowBitsBytes = 48u << 10;  // LDS k_mq_row_bits may take for a row's bits

static_assert(sizeof(fs_misquote) == 32 && sizeof(fs_misquote_pair) == 32 &&
              sizeof(fs_misquote_work) == 32, "fs_misquotes");
static_assert(offsetof(fs_misquote_work, passage_records) == 0 &&
              offsetof(fs_misquote_work, departures) == 4 &&
              offsetof(fs_misquote_work, misquotes) == 8 &&
              offsetof(fs_misquote_work, telling) == 12 &&
              offsetof(fs_misquote_work, singular) == 16 &&
              offsetof(fs_misquote_work, partners) == 20, "fs_misquote_work");

typedef unsigned long long u64;

struct MqArgs {
  const uint32_t* work;
  const uint32_t* orig;
  const uint32_t* spell;
  const uint32_t* same;          // [n_script]
  const uint32_t* heads;         // [n_runs + 1]
  uint32_t n, n_runs, n_works, n_script, n_spell;
  uint32_t min_words, min_works, max_share, flat, min_shared, min_score;
  uint32_t n_listed, n_post, n_pairs;
  uint64_t n_contrib;            // P
  uint64_t mask;                 // slots - 1 of each of the three record tables
  uint64_t pmask;                // slots - 1 of the pair table
  uint64_t hash_mask;            // FS_MISQUOTES_HASH_BITS: the bits of every hash kept
  u64* ow_tab;                   // orig_ix << 32 | work: the readers
  u64* cell_tab;                 // orig_ix << 32 | spell: the misquotes
  u64* cw_tab;                   // cell slot << 32 | work
  uint32_t* cell_rec;            // [slots] departures of the cell in that slot
  uint32_t* cell_works;          //         its works
  uint32_t* cell_first;          //         its smallest work
  uint32_t* cell_ix;             //         its number once listed (FS_NONE: not listed)
  uint32_t* readers;             // [n_script]
  uint32_t* lcnt;                // [n_script] listed cells of the word
  uint32_t* lfirst;              //            those of the words in front
  uint32_t* lcur;                //            placed so far
  uint32_t* ltmp;                // [n_listed] cell slots, word by word, unranked
  uint32_t* t_off;               // [n_listed] works of the telling misquotes in front
  uint32_t* t_cur;               //            works placed: the list's length afterwards
  u64* p_off;                    // [n_listed] contributions of the misquotes in front
  uint32_t* w_off;               // [n_works] telling misquotes of the works in front
  uint32_t* w_cur;               //           placed: the list's length afterwards
  uint2* t_ent;                  // [n_post] {work, misquote} unranked
  uint2* w_ent;                  // [n_post] {misquote, work} unranked
  uint32_t* t_post;              // [n_post] works of every telling misquote, ascending
  uint32_t* w_post;              // [n_post] telling misquotes of every work, ascending
  u64* pkey;                     // [pair slots] a << 32 | b
  uint32_t* pshared;             //
  uint32_t* pscore;              //
  u64* pstrong;                  //              weight << 32 | (0xFFFFFFFF - number)
  uint32_t* r_cnt;               // [n_works] kept pairs with a = the work
  uint32_t* r_off;               //           those of the works in front
  uint32_t* r_cur;               //           placed
  uint2* r_ent;                  // [n_pairs] {b, a} unranked
  uint32_t* r_pay;               // [n_pairs] their slots
  uint32_t* r_slot;              // [n_pairs] the slots in (a, b) order
  u64* close;                    // [n_works] score << 32 | ~partner
  uint32_t* status;              // [0] invalid input, [1] total of the last 32-bit scan, [2] active works
  u64* total;                    // [0] P
  fs_misquote_work* works;
  fs_misquote* mis;
  fs_misquote_pair* pairs;
};

// the slot of `key` in `tab`; true when this call put it there
__device__ inline bool set_insert(u64* tab, uint64_t mask, uint64_t hash_mask, u64 key,
                                  uint64_t* slot) {
  bool inserted;
  *slot = fs_probe_insert(tab, mask, fs_mix64(key) & hash_mask, key,
                          [key](u64 cur) { return cur == key; }, &inserted);
  return inserted;
}

// `key` is in `tab` (no insert runs beside this)
__device__ inline bool set_has(const u64* __restrict__ tab, uint64_t mask, uint64_t hash_mask,
                               u64 key) {
  for (uint64_t pos = fs_mix64(key) & hash_mask & mask;; pos = (pos + 1) & mask) {
    const u64 cur = tab[pos];
    if (cur == key) return true;
    if (cur == kProbeEmpty) return false;
  }
}

__global__ __launch_bounds__(kBlock) void k_mq_check(MqArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool bad = i < a.n && (a.work[i] >= a.n_works || a.orig[i] >= a.n_script ||
                               a.spell[i] >= a.n_spell);
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 1u);
}

__global__ __launch_bounds__(kBlock) void k_mq_same(MqArgs a) {
  const uint32_t o = blockIdx.x * kBlock + threadIdx.x;
  const bool bad = o < a.n_script && a.same[o] != FS_NONE && a.same[o] >= a.n_spell;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 2u);
}

__global__ __launch_bounds__(kBlock) void k_mq_cells(MqArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  uint32_t lo = 0, hi = a.n_runs;                  // the run of i: heads[lo] <= i < heads[lo + 1]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.heads[mid] <= i) lo = mid; else hi = mid;
  }
  if (a.heads[lo + 1] - a.heads[lo] < a.min_words) return;
  const uint32_t w = a.work[i], o = a.orig[i], s = a.spell[i];
  uint32_t* __restrict__ wc = reinterpret_cast<uint32_t*>(a.works + w);
  uint64_t cell, other;
  atomicAdd(&wc[0], 1u);
  if (set_insert(a.ow_tab, a.mask, a.hash_mask, (u64)o << 32 | w, &other))
    atomicAdd(&a.readers[o], 1u);
  if (s == a.same[o]) return;
  atomicAdd(&wc[1], 1u);
  set_insert(a.cell_tab, a.mask, a.hash_mask, (u64)o << 32 | s, &cell);
  atomicAdd(&a.cell_rec[cell], 1u);
  if (set_insert(a.cw_tab, a.mask, a.hash_mask, (u64)cell << 32 | w, &other))
    atomicAdd(&a.cell_works[cell], 1u);
  // a value read here is never below the slot's final one: a work at or above it need not try
  if (w < ld_agent(&a.cell_first[cell])) atomicMin(&a.cell_first[cell], w);
}

// the weight of a listed cell of k works at a word of `readers` readers; 0: not telling
__device__ inline uint32_t weight_of(const MqArgs& a, uint32_t k, uint32_t readers) {
  if ((uint64_t)k * 100 > (uint64_t)a.max_share * readers) return 0;
  return a.flat ? 1u : 32u - (uint32_t)__clz((int)(readers / k));
}

// cell_ix: 0 for a listed cell until k_mq_number numbers it, FS_NONE for the others
__global__ __launch_bounds__(kBlock) void k_mq_classify(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const u64 key = a.cell_tab[slot];
  if (key == kProbeEmpty || a.cell_works[slot] < a.min_works) return;
  a.cell_ix[slot] = 0;
  atomicAdd(&a.lcnt[(uint32_t)(key >> 32)], 1u);
}

// exclusive scan of in[0..n) into out (which may be in), *total = the sum
__global__ __launch_bounds__(kScanBlock) void k_mq_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t n, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, n, out, total);
}

__global__ __launch_bounds__(kBlock) void k_mq_scatter(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const u64 key = a.cell_tab[slot];
  if (key == kProbeEmpty || a.cell_ix[slot] == FS_NONE) return;
  const uint32_t o = (uint32_t)(key >> 32);
  a.ltmp[a.lfirst[o] + atomicAdd(&a.lcur[o], 1u)] = (uint32_t)slot;
}

// {works, records, spell} of x stand in front of those of y inside their word
__device__ inline bool precedes(uint32_t xw, uint32_t xr, uint32_t xs, uint32_t yw, uint32_t yr,
                                uint32_t ys) {
  if (xw != yw) return xw > yw;
  if (xr != yr) return xr > yr;
  return xs < ys;
}

__device__ inline bool slot_precedes(const MqArgs& a, uint32_t x, uint32_t yw, uint32_t yr,
                                     uint32_t ys) {
  return precedes(a.cell_works[x], a.cell_rec[x], (uint32_t)a.cell_tab[x], yw, yr, ys);
}

// one lane per listed cell: the listed cells of its word that precede it are its place there
__global__ __launch_bounds__(kBlock) void k_mq_number(MqArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool live = p < a.n_listed;
  uint32_t slot = 0, o = 0, cw = 0, cr = 0, cs = 0, first = 0, len = 0, rank = 0;
  if (live) {
    slot = a.ltmp[p];
    const u64 key = a.cell_tab[slot];
    o = (uint32_t)(key >> 32);
    cs = (uint32_t)key;
    cw = a.cell_works[slot];
    cr = a.cell_rec[slot];
    first = a.lfirst[o];
    len = a.lcnt[o];
  }
  const bool is_long = live && len > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = lane_u32(first, j), lj = lane_u32(len, j);
    const uint32_t wj = lane_u32(cw, j), rj = lane_u32(cr, j), sj = lane_u32(cs, j);
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64)
      before += slot_precedes(a, a.ltmp[fj + k], wj, rj, sj) ? 1u : 0u;
    before = wave_sum(before);
    if (lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k)
      rank += slot_precedes(a, a.ltmp[first + k], cw, cr, cs) ? 1u : 0u;
  if (live) {
    const uint32_t readers = a.readers[o];
    const uint32_t wt = weight_of(a, cw, readers);
    a.cell_ix[slot] = first + rank;
    a.mis[first + rank] = fs_misquote{o, cs, cr, cw, readers, wt ? 1u : 0u, wt, a.cell_first[slot]};
  }
}

// one lane per (cell, work): what the work's row of the table counts
__global__ __launch_bounds__(kBlock) void k_mq_count(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const u64 key = a.cw_tab[slot];
  if (key == kProbeEmpty) return;
  const uint32_t cell = (uint32_t)(key >> 32);
  uint32_t* __restrict__ wc = reinterpret_cast<uint32_t*>(a.works + (uint32_t)key);
  if (a.cell_works[cell] == 1) atomicAdd(&wc[4], 1u);
  const uint32_t m = a.cell_ix[cell];
  if (m == FS_NONE) return;
  atomicAdd(&wc[2], 1u);
  if (a.mis[m].weight) atomicAdd(&wc[3], 1u);
}

// One workgroup, three scans in turn: the works of the telling misquotes in front of each
// misquote (status[1] = their sum), the contributions in front of it in 64 bits (total[0] = P),
// the telling misquotes of the works in front of each work; status[2] = the active works.
__global__ __launch_bounds__(kScanBlock) void k_mq_offsets(MqArgs a) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  __shared__ u64 s_p[kScanBlock / 64];
  const uint32_t posts = scan_chunks<1, uint32_t, uint32_t>(
      a.n_listed, [&a](uint64_t m) { return a.mis[m].weight ? a.mis[m].works : 0u; },
      [&a](uint64_t m, uint32_t at, uint32_t) { a.t_off[m] = at; }, s_w);
  __syncthreads();
  const u64 contrib = scan_chunks<1, u64, u64>(
      a.n_listed,
      [&a](uint64_t m) {
        const u64 k = a.mis[m].works;
        return a.mis[m].weight ? k * (k - 1) / 2 : 0ull;
      },
      [&a](uint64_t m, u64 at, u64) { a.p_off[m] = at; }, s_p);
  __syncthreads();
  scan_chunks<1, uint32_t, uint32_t>(
      a.n_works, [&a](uint64_t w) { return a.works[w].telling; },
      [&a](uint64_t w, uint32_t at, uint32_t) { a.w_off[w] = at; }, s_w);
  uint32_t active = 0;
  for (uint32_t w = threadIdx.x; w < a.n_works; w += kScanBlock)
    active += a.works[w].passage_records ? 1u : 0u;
  active = wave_sum(active);
  if ((threadIdx.x & 63) == 0 && active) atomicAdd(&a.status[2], active);
  if (threadIdx.x == 0) {
    a.status[1] = posts;
    a.total[0] = contrib;
  }
}

__global__ __launch_bounds__(kBlock) void k_mq_post(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const u64 key = a.cw_tab[slot];
  if (key == kProbeEmpty) return;
  const uint32_t w = (uint32_t)key, m = a.cell_ix[(uint32_t)(key >> 32)];
  if (m == FS_NONE || !a.mis[m].weight) return;
  a.t_ent[a.t_off[m] + atomicAdd(&a.t_cur[m], 1u)] = make_uint2(w, m);
  a.w_ent[a.w_off[w] + atomicAdd(&a.w_cur[w], 1u)] = make_uint2(m, w);
}

// Entries {key, list}, list by list (list l at off[l], len[l] of them, keys all different): one
// lane per entry, the keys of its list below its own are its place there.  out (if any) takes
// the keys, out_pay (if any) the entry's pay[].  The lists of more than `most` entries are left
// alone (k_mq_row_bits places them).
__global__ __launch_bounds__(kBlock) void k_mq_rank(const uint2* __restrict__ ent, uint32_t n,
                                                    const uint32_t* __restrict__ off,
                                                    const uint32_t* __restrict__ len,
                                                    uint32_t* __restrict__ out,
                                                    const uint32_t* __restrict__ pay,
                                                    uint32_t* __restrict__ out_pay, uint32_t most) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  bool live = p < n;
  uint2 e = make_uint2(0, 0);
  uint32_t first = 0, l = 0, rank = 0;
  if (live) {
    e = ent[p];
    first = off[e.y];
    l = len[e.y];
    live = l <= most;
  }
  const bool is_long = live && l > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = lane_u32(first, j), lj = lane_u32(l, j), xj = lane_u32(e.x, j);
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) before += ent[fj + k].x < xj ? 1u : 0u;
    before = wave_sum(before);
    if (lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < l; ++k) rank += ent[first + k].x < e.x ? 1u : 0u;
  if (live) {
    if (out) out[first + rank] = e.x;
    if (out_pay) out_pay[first + rank] = pay[p];
  }
}

// Contribution t of P: the list m with p_off[m] <= t < p_off[m] + k (k - 1) / 2, and inside it
// the pair (i < j) with j (j - 1) / 2 + i = t - p_off[m].  A list of five thousand works and a
// thousand lists of two load the lanes alike: a lane has one contribution.
__global__ __launch_bounds__(kBlock) void k_mq_expand(MqArgs a) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= a.n_contrib) return;
  uint32_t lo = 0, hi = a.n_listed;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a.p_off[mid] <= t) lo = mid; else hi = mid;
  }
  const uint32_t m = lo;
  const uint64_t r = t - a.p_off[m];
  // a double's square root seeds j; the integer comparisons decide
  uint64_t j = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)r)) * 0.5);
  if (j < 1) j = 1;
  while (j * (j - 1) / 2 > r) --j;
  while ((j + 1) * j / 2 <= r) ++j;
  const uint64_t i = r - j * (j - 1) / 2;
  const uint32_t base = a.t_off[m];
  const uint32_t wa = a.t_post[base + i], wb = a.t_post[base + j];     // ascending: wa < wb
  const uint32_t wt = a.mis[m].weight;
  uint64_t slot;
  set_insert(a.pkey, a.pmask, a.hash_mask, (u64)wa << 32 | wb, &slot);
  atomicAdd(&a.pshared[slot], 1u);
  atomicAdd(&a.pscore[slot], wt);
  const u64 strong = (u64)wt << 32 | (FS_NONE - m);
  if (strong > __hip_atomic_load(&a.pstrong[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(&a.pstrong[slot], strong);
}

__device__ inline bool kept(const MqArgs& a, uint64_t slot) {
  return a.pkey[slot] != kProbeEmpty && a.pshared[slot] >= a.min_shared &&
         a.pscore[slot] >= a.min_score;
}

__global__ __launch_bounds__(kBlock) void k_mq_keep(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.pmask || !kept(a, slot)) return;
  const u64 key = a.pkey[slot];
  const uint32_t wa = (uint32_t)(key >> 32), wb = (uint32_t)key;
  const u64 score = (u64)a.pscore[slot] << 32;
  atomicAdd(&a.works[wa].partners, 1u);
  atomicAdd(&a.works[wb].partners, 1u);
  atomicMax(&a.close[wa], score | (uint32_t)~wb);
  atomicMax(&a.close[wb], score | (uint32_t)~wa);
  atomicAdd(&a.r_cnt[wa], 1u);
}

__global__ __launch_bounds__(kBlock) void k_mq_rows(MqArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.pmask || !kept(a, slot)) return;
  const u64 key = a.pkey[slot];
  const uint32_t wa = (uint32_t)(key >> 32);
  const uint32_t at = a.r_off[wa] + atomicAdd(&a.r_cur[wa], 1u);
  a.r_ent[at] = make_uint2((uint32_t)key, wa);
  a.r_pay[at] = (uint32_t)slot;
}

// One workgroup per work with more than kLong kept partners: a bit per partner in LDS (`words`
// 32-bit words cover every work number), the set bits in front of every thread's stretch of
// words by a scan, and a partner's place in the row is the number of set bits below its own.
// Linear in the row where k_mq_rank compares every two entries of it.
__global__ __launch_bounds__(kBlock) void k_mq_row_bits(MqArgs a, uint32_t words) {
  extern __shared__ uint32_t s_bits[];           // [words]
  __shared__ uint32_t s_pre[kBlock];             // set bits in front of thread t's stretch
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t wa = blockIdx.x;
  const uint32_t len = a.r_cur[wa];
  if (len <= kLong) return;                      // (the whole workgroup)
  const uint32_t first = a.r_off[wa];
  for (uint32_t k = threadIdx.x; k < words; k += kBlock) s_bits[k] = 0;
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < len; k += kBlock) {
    const uint32_t b = a.r_ent[first + k].x;
    atomicOr(&s_bits[b >> 5], 1u << (b & 31));
  }
  __syncthreads();
  const uint32_t stretch = (words + kBlock - 1) / kBlock;
  const uint32_t w0 = threadIdx.x * stretch;
  uint32_t mine = 0, total;
  for (uint32_t k = w0; k < w0 + stretch && k < words; ++k) mine += (uint32_t)__popc(s_bits[k]);
  s_pre[threadIdx.x] = block_scan<kBlock>(mine, s_w, &total);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < len; k += kBlock) {
    const uint32_t b = a.r_ent[first + k].x, word = b >> 5;
    uint32_t rank = s_pre[word / stretch] + (uint32_t)__popc(s_bits[word] & ((1u << (b & 31)) - 1));
    for (uint32_t j = word / stretch * stretch; j < word; ++j) rank += (uint32_t)__popc(s_bits[j]);
    a.r_slot[first + rank] = a.r_pay[first + k];
  }
}

__global__ __launch_bounds__(kBlock) void k_mq_finish(MqArgs a) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w >= a.n_works) return;
  const bool any = a.works[w].partners != 0;
  const u64 c = a.close[w];
  a.works[w].closest = any ? ~(uint32_t)c : FS_NONE;
  a.works[w].closest_score = any ? (uint32_t)(c >> 32) : 0u;
}

// the telling misquotes of `mine` at script words `other` reads
__device__ inline uint32_t on_common(const MqArgs& a, uint32_t mine, uint32_t other) {
  uint32_t n = 0;
  const uint32_t first = a.w_off[mine], len = a.w_cur[mine];
  for (uint32_t k = 0; k < len; ++k) {
    const uint32_t o = a.mis[a.w_post[first + k]].orig_ix;
    n += set_has(a.ow_tab, a.mask, a.hash_mask, (u64)o << 32 | other) ? 1u : 0u;
  }
  return n;
}

__global__ __launch_bounds__(kBlock) void k_mq_detail(MqArgs a) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= a.n_pairs) return;
  const uint32_t slot = a.r_slot[q];
  const u64 key = a.pkey[slot], strong = a.pstrong[slot];
  const uint32_t wa = (uint32_t)(key >> 32), wb = (uint32_t)key;
  a.pairs[q] = fs_misquote_pair{wa, wb, a.pshared[slot], a.pscore[slot], on_common(a, wa, wb),
                                on_common(a, wb, wa), FS_NONE - (uint32_t)strong,
                                (uint32_t)(strong >> 32)};
}

uint64_t misquotes_hash_mask() {
  const char* e = getenv("FS_MISQUOTES_HASH_BITS");  // diagnostic: k bits of the hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1;
}

// the most contributions a call takes: what FS_MISQUOTES_MAX_BYTES admits, or fewer
uint64_t misquotes_max_pairs() {
  const uint64_t most = FS_MISQUOTES_MAX_BYTES / FS_MISQUOTES_SLOT_BYTES / 2;
  const char* e = getenv("FS_MISQUOTES_MAX_PAIRS");
  if (!e || !*e) return most;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return v < most ? v : most;
}

struct RunsGuard {
  fs_runs* r = nullptr;
  ~RunsGuard() { if (r) fs_runs_free(r); }
};

// passages, cells, number, postings, expand, place, detail, total of the last call
thread_local double t_ms[8];

template <class T>
int filled(DBuf<T>& d, size_t count, int byte = 0) {
  FS_TRY(d.reserve(count));
  if (count) FS_HIP(hipMemsetAsync(d.p, byte, count * sizeof(T), nullptr));
  return FS_OK;
}

#define MQ_LAUNCH(kernel, count, ...)                                                          \
  do {                                                                                         \
    if (count)                                                                                 \
      hipLaunchKernelGGL(kernel, dim3(blocks_of(count, kBlock)), dim3(kBlock), 0, nullptr,     \
                         __VA_ARGS__);                                                         \
  } while (0)

}  // namespace

extern "C" int fs_misquotes(int device, const uint32_t* work, const uint32_t* fan_ix,
                            const uint32_t* orig_ix, const uint32_t* spell, const uint32_t* same,
                            uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t n_spell,
                            uint32_t min_words, uint32_t max_gap, uint32_t min_works,
                            uint32_t max_share, uint32_t weight, uint32_t min_shared,
                            uint32_t min_score, fs_misquote_work* works, fs_misquote* misquotes,
                            uint64_t cap_m, uint64_t* n_misquotes, fs_misquote_pair* pairs,
                            uint64_t cap_p, uint64_t* n_pairs) {
  for (double& t : t_ms) t = 0.0;
  if (!n_misquotes || !n_pairs || (n_works && !works) || (cap_m && !misquotes) ||
      (cap_p && !pairs)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_works < 2 || max_share < 1 || max_share > 100 || min_shared == 0 ||
      min_score == 0 || weight > FS_MISQUOTES_FLAT) {
    fs_set_error("min_words, min_shared and min_score must be at least 1, min_works at least 2, "
                 "max_share from 1 to 100, weight FS_MISQUOTES_RARITY or FS_MISQUOTES_FLAT");
    return FS_E_INVALID;
  }
  if (n_rows >= kMaxRows) {
    fs_set_error("%llu records: misquotes take fewer than 2^27 (a score is 32 bits)",
                 (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(record_limits("misquotes", n_rows, n_script));
  *n_misquotes = *n_pairs = 0;
  if (n_rows == 0) {
    for (uint32_t w = 0; w < n_works; ++w) works[w] = fs_misquote_work{0, 0, 0, 0, 0, 0, FS_NONE, 0};
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix || !spell || !same) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  const auto invalid = [](uint32_t st) {
    fs_set_error(st & 1u ? "a work >= n_works, an orig_ix >= n_script or a spell >= n_spell"
                         : "a same[] that is neither 0xFFFFFFFF nor below n_spell");
    return FS_E_INVALID;
  };
  if (!n_works || !n_script || !n_spell) return invalid(1);
  const uint32_t n = (uint32_t)n_rows;
  const uint64_t slots = fs_probe_slots(n);
  if (slots * FS_MISQUOTES_RECORD_SLOT_BYTES > FS_MISQUOTES_MAX_BYTES) {
    fs_set_error("%u records: record tables of more than %u bytes", n, FS_MISQUOTES_MAX_BYTES);
    return FS_E_UNSUPPORTED;
  }
  const uint64_t max_pairs = misquotes_max_pairs();
  FS_ENTER(device);

  // ---- passages: the records checked, the run heads
  DBuf<uint32_t> d_work, d_fan, d_orig, d_spell, d_same, d_status;
  DBuf<u64> d_total;
  DBuf<fs_misquote_work> d_works;
  FS_TRY(d_work.upload(work, n, nullptr));
  FS_TRY(d_fan.upload(fan_ix, n, nullptr));
  FS_TRY(d_orig.upload(orig_ix, n, nullptr));
  FS_TRY(d_spell.upload(spell, n, nullptr));
  FS_TRY(d_same.upload(same, n_script, nullptr));
  FS_TRY(filled(d_status, 4));
  FS_TRY(filled(d_total, 1));
  FS_TRY(filled(d_works, n_works));
  MqArgs a{};
  a.work = d_work.p;
  a.orig = d_orig.p;
  a.spell = d_spell.p;
  a.same = d_same.p;
  a.n = n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.n_spell = n_spell;
  a.min_words = min_words;
  a.min_works = min_works;
  a.max_share = max_share;
  a.flat = weight == FS_MISQUOTES_FLAT;
  a.min_shared = min_shared;
  a.min_score = min_score;
  a.hash_mask = misquotes_hash_mask();
  a.status = d_status.p;
  a.total = d_total.p;
  a.works = d_works.p;
  Clock<8> clk;
  FS_TRY(clk.mark(0, nullptr));
  MQ_LAUNCH(k_mq_check, n, a);
  MQ_LAUNCH(k_mq_same, n_script, a);
  FS_HIP(hipGetLastError());
  RunsGuard runs;
  FS_TRY(fs_runs_find_cols(d_work.p, d_fan.p, d_orig.p, n, min_words, max_gap, nullptr, &runs.r,
                           &a.heads, &a.n_runs));
  uint32_t st[2];
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) return invalid(st[0]);
  FS_TRY(clk.mark(1, nullptr));

  // ---- cells: readers, misquotes and their works
  DBuf<u64> d_keys;                              // the three key tables
  DBuf<uint32_t> d_cell, d_first, d_ix;          // cell_rec and cell_works; cell_first; cell_ix
  DBuf<uint32_t> d_word;                         // readers, lcnt, lfirst, lcur
  FS_TRY(filled(d_keys, 3 * slots, 0xFF));
  FS_TRY(filled(d_cell, 2 * slots));
  FS_TRY(filled(d_first, slots, 0xFF));
  FS_TRY(filled(d_ix, slots, 0xFF));
  FS_TRY(filled(d_word, 4 * (size_t)n_script));
  a.mask = slots - 1;
  a.ow_tab = d_keys.p;
  a.cell_tab = d_keys.p + slots;
  a.cw_tab = d_keys.p + 2 * slots;
  a.cell_rec = d_cell.p;
  a.cell_works = d_cell.p + slots;
  a.cell_first = d_first.p;
  a.cell_ix = d_ix.p;
  a.readers = d_word.p;
  a.lcnt = d_word.p + n_script;
  a.lfirst = d_word.p + 2 * (size_t)n_script;
  a.lcur = d_word.p + 3 * (size_t)n_script;
  MQ_LAUNCH(k_mq_cells, n, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(2, nullptr));

  // ---- number: the listed misquotes in the order of their key, the works' counts
  MQ_LAUNCH(k_mq_classify, slots, a);
  hipLaunchKernelGGL(k_mq_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.lcnt, a.lfirst, n_script,
                     a.status + 1);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  a.n_listed = st[1];
  *n_misquotes = a.n_listed;
  DBuf<uint32_t> d_ltmp, d_list;                 // ltmp; t_off, t_cur
  DBuf<u64> d_poff;
  DBuf<uint32_t> d_wlist;                        // w_off, w_cur
  DBuf<fs_misquote> d_mis;
  FS_TRY(d_ltmp.reserve(a.n_listed));
  FS_TRY(filled(d_list, 2 * (size_t)a.n_listed));
  FS_TRY(d_poff.reserve(a.n_listed));
  FS_TRY(filled(d_wlist, 2 * (size_t)n_works));
  FS_TRY(d_mis.reserve(a.n_listed));
  a.ltmp = d_ltmp.p;
  a.t_off = d_list.p;
  a.t_cur = d_list.p + a.n_listed;
  a.p_off = d_poff.p;
  a.w_off = d_wlist.p;
  a.w_cur = d_wlist.p + n_works;
  a.mis = d_mis.p;
  MQ_LAUNCH(k_mq_scatter, slots, a);
  MQ_LAUNCH(k_mq_number, a.n_listed, a);
  MQ_LAUNCH(k_mq_count, slots, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(3, nullptr));

  // ---- postings: the works of every telling misquote, the telling misquotes of every work
  hipLaunchKernelGGL(k_mq_offsets, dim3(1), dim3(kScanBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  uint32_t st2[3];
  FS_HIP(hipMemcpy(st2, d_status.p, sizeof st2, hipMemcpyDeviceToHost));
  FS_HIP(hipMemcpy(&a.n_contrib, d_total.p, sizeof(u64), hipMemcpyDeviceToHost));
  a.n_post = st2[1];
  // the active works bound the pairs there can be; the table is sized before it is allocated
  const uint64_t n_active = st2[2];
  const uint64_t all_pairs = n_active ? n_active * (n_active - 1) / 2 : 0;
  const uint64_t keys = a.n_contrib < all_pairs ? a.n_contrib : all_pairs;
  if (a.n_contrib > max_pairs) {
    fs_set_error("P = %llu contributions of the telling misquotes, more than %llu: a smaller "
                 "--max-share leaves out the misquotes most works share",
                 (unsigned long long)a.n_contrib, (unsigned long long)max_pairs);
    return FS_E_UNSUPPORTED;
  }
  DBuf<uint2> d_ent;                             // t_ent, w_ent
  DBuf<uint32_t> d_post;                         // t_post, w_post
  FS_TRY(d_ent.reserve(2 * (size_t)a.n_post));
  FS_TRY(d_post.reserve(2 * (size_t)a.n_post));
  a.t_ent = d_ent.p;
  a.w_ent = d_ent.p + a.n_post;
  a.t_post = d_post.p;
  a.w_post = d_post.p + a.n_post;
  MQ_LAUNCH(k_mq_post, slots, a);
  MQ_LAUNCH(k_mq_rank, a.n_post, a.t_ent, a.n_post, a.t_off, a.t_cur, a.t_post, nullptr, nullptr,
            FS_NONE);
  MQ_LAUNCH(k_mq_rank, a.n_post, a.w_ent, a.n_post, a.w_off, a.w_cur, a.w_post, nullptr, nullptr,
            FS_NONE);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, nullptr));

  // ---- expand: every telling list into its pairs
  const uint64_t pslots = fs_probe_slots(keys);
  DBuf<u64> d_pk;                                // pkey; pstrong
  DBuf<uint32_t> d_pc;                           // pshared, pscore
  DBuf<uint32_t> d_row;                          // r_cnt, r_off, r_cur
  DBuf<u64> d_close;
  FS_TRY(d_pk.reserve(2 * pslots));
  FS_HIP(hipMemsetAsync(d_pk.p, 0xFF, pslots * sizeof(u64), nullptr));
  FS_HIP(hipMemsetAsync(d_pk.p + pslots, 0, pslots * sizeof(u64), nullptr));
  FS_TRY(filled(d_pc, 2 * pslots));
  FS_TRY(filled(d_row, 3 * (size_t)n_works));
  FS_TRY(filled(d_close, n_works));
  a.pmask = pslots - 1;
  a.pkey = d_pk.p;
  a.pstrong = d_pk.p + pslots;
  a.pshared = d_pc.p;
  a.pscore = d_pc.p + pslots;
  a.r_cnt = d_row.p;
  a.r_off = d_row.p + n_works;
  a.r_cur = d_row.p + 2 * (size_t)n_works;
  a.close = d_close.p;
  MQ_LAUNCH(k_mq_expand, a.n_contrib, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(5, nullptr));

  // ---- place: the keep rule, partners and closest, the kept pairs in (a, b) order
  MQ_LAUNCH(k_mq_keep, pslots, a);
  hipLaunchKernelGGL(k_mq_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.r_cnt, a.r_off, n_works,
                     a.status + 1);
  MQ_LAUNCH(k_mq_finish, n_works, a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  a.n_pairs = st[1];
  *n_pairs = a.n_pairs;
  FS_TRY(copy_out(works, d_works, n_works));
  if (a.n_listed > cap_m || a.n_pairs > cap_p) {
    fs_set_error("%u misquotes and %u pairs need room", a.n_listed, a.n_pairs);
    return FS_E_CAPACITY;
  }
  DBuf<uint2> d_rent;
  DBuf<uint32_t> d_rs;                           // r_pay, r_slot
  DBuf<fs_misquote_pair> d_pairs;
  FS_TRY(d_rent.reserve(a.n_pairs));
  FS_TRY(d_rs.reserve(2 * (size_t)a.n_pairs));
  FS_TRY(d_pairs.reserve(a.n_pairs));
  a.r_ent = d_rent.p;
  a.r_pay = d_rs.p;
  a.r_slot = d_rs.p + a.n_pairs;
  a.pairs = d_pairs.p;
  MQ_LAUNCH(k_mq_rows, pslots, a);
  // a long row by its bits in LDS when a bit per work fits there, else by k_mq_rank as well
  const uint32_t row_words = (n_works + 31) / 32;
  const bool by_bits = (size_t)row_words * sizeof(uint32_t) <= kRowBitsBytes;
  MQ_LAUNCH(k_mq_rank, a.n_pairs, a.r_ent, a.n_pairs, a.r_off, a.r_cur, nullptr, a.r_pay, a.r_slot,
            by_bits ? kLong : FS_NONE);
  if (by_bits && a.n_pairs > kLong)
    hipLaunchKernelGGL(k_mq_row_bits, dim3(n_works), dim3(kBlock),
                       row_words * sizeof(uint32_t), nullptr, a, row_words);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(6, nullptr));

  // ---- detail: what each work of a kept pair departs in on the ground both quote
  MQ_LAUNCH(k_mq_detail, a.n_pairs, a);
  FS_HIP(hipGetLastError());
  if (a.n_listed) FS_TRY(copy_out(misquotes, d_mis, a.n_listed));
  if (a.n_pairs) FS_TRY(copy_out(pairs, d_pairs, a.n_pairs));
  FS_TRY(clk.mark(7, nullptr));
  FS_HIP(hipDeviceSynchronize());
  for (int k = 0; k < 7; ++k) t_ms[k] = clk.elapsed(k, k + 1);
  t_ms[7] = clk.elapsed(0, 7);
  return FS_OK;
}

extern "C" int fs_misquotes_times(double* ms) {
  return times_out(ms, t_ms, 8);
}
