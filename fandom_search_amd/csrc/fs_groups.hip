// fs_groups.hip -- `ao3.py groups`: match records reduced by groups of works (fs_groups,
// fs_groups_rows in include/fandom_search.h).  Membership is many-to-many, and the figures per
// group are distinct counts: the depth of a script word is a column sum over the coverage rows
// of the group's works.
//
// The membership arrives on the host and is turned group-major there (a counting sort, one pass
// over the memberships), cut into units: a unit is a slab of at most kSplit works of one
// group.  A group of up to kSplit works is one unit; a larger one is split over several, whose
// partial sums meet in one atomic each.  Every kernel below takes a lane per (unit, item), so
// one group of all works is many units side by side and a hundred thousand groups of one work
// are lanes, not waves.  Every output is an integer; separate launches, no workgroup waits on
// another:
//   fs_runs_find      the run heads of fs_passages.hip (and its sortedness check)
//   k_groups_records  one lane per record: bounds; records and exact records per work and per
//                     (work, label), one atomic per distinct key of a wave
//   k_groups_runs     one lane per run: a kept run into its work's passage figures and, through
//                     fs_cover_span (fs_cover.h), into its work's coverage row
//   k_groups_stats    one lane per unit: the works' figures summed in registers
//   k_groups_labels   one lane per (unit, label): records per label summed over the slab
//   k_groups_depth<0> one lane per (unit, 64 script words): the slab's coverage words added
//                     into eight bit planes, a column count per bit.  A one-unit group is
//                     finished from the planes; a split one adds its non-zero counts to its
//                     depth row
//   k_groups_big<0>   one lane per (split group, 64 script words): the same figures from the row
//   k_groups_cells<0> one lane per (group, label): cells per block of 64 labels, the top label
//   k_groups_finish   one lane per group: peak and top label unpacked
//   k_groups_scan     one workgroup, twice: where a group's cells and word rows go
//   k_groups_depth<1>, k_groups_big<1>, k_groups_cells<1>   the place pass: the same figures
//                     again, every row written behind the rows in front of it
// The lanes of a unit are padded to whole segments (64, or the power of two above a smaller
// item count), so that a segment never straddles two units and sums, maxima and prefixes inside
// it are shuffles.
#include "fs_internal.h"
#include "fs_cover.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kPlanes = 8;
constexpr uint32_t kSplit = 255;            // works per unit: what kPlanes bits count (tests: SPLIT)
constexpr uint32_t kGroupWords = sizeof(fs_group) / 4;
enum { G_WORKS, G_PWORKS, G_WORDS, G_EXACT, G_PASSAGES, G_PASSAGE_WORDS, G_LONGEST, G_COVERED,
       G_PEAK, G_PEAK_FIRST, G_TOP, G_TOP_WORDS, G_CELLS, G_ROWS };
constexpr uint32_t kWorkStats = 5;          // records, exact, passages, records in them, longest

struct GroupsArgs {
  uint32_t n, n_works, n_script, nk, n_groups, n_labels, n_runs, min_words, min_works;
  uint32_t seg_k, nkp, nkb;     // lanes of a unit over the 64-bit words: segment, padded, blocks
  uint32_t seg_l, nlp, nlb;     // lanes of a group over the labels
  uint32_t n_units, n_split;
  const uint32_t* heads;        // [n_runs + 1]
  const uint32_t* label_of;     // [n_script]
  const uint4* units;           // [n_units] {group, first member, one past the last, depth row or FS_NONE}
  const uint32_t* members;      // the works, group-major
  const uint32_t* split_group;  // [n_split] group of a depth row
  uint32_t* wstat;              // [n_works][kWorkStats]
  uint2* wl;                    // [n_works][n_labels] {records, exact}
  unsigned long long* cov;      // [n_works][nk]
  uint32_t* depth;              // [n_split][nk * 64]
  uint32_t* glw;                // [n_groups][n_labels] records, ...
  uint32_t* glx;                //   exact records, ...
  uint32_t* glm;                //   works
  uint32_t* cbw;                // [n_groups][nkb] word rows of a block of 64 x 64 script words
  uint32_t* cbl;                // [n_groups][nlb] cells of a block of 64 labels
  unsigned long long* gpeak;    // [n_groups] depth << 32 | (0xFFFFFFFF - word)
  unsigned long long* gtop;     // [n_groups] records << 32 | (0xFFFFFFFF - label)
  unsigned long long* woff;     // [n_groups] first word row
  unsigned long long* coff;     // [n_groups] first cell
  uint32_t* status;             // [0] invalid input
  uint32_t* groups;             // fs_group[n_groups] as words
  fs_group_cell* cells;
  fs_group_word* words;
};

__device__ inline unsigned long long lane_value64(unsigned long long v, int lane) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// Called by the whole wave: the lanes of `todo` that carry the key of its first lane.
__device__ inline uint64_t same_key(uint64_t todo, bool valid, unsigned long long key,
                                    int* first, unsigned long long* kf) {
  *first = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
  *kf = lane_value64(key, *first);
  return __ballot(valid && key == *kf) & todo;
}

// sums, maxima and exclusive prefixes inside aligned segments of `seg` lanes (a power of two)
__device__ inline uint32_t seg_sum(uint32_t v, uint32_t seg) {
  for (uint32_t d = 1; d < seg; d <<= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ inline unsigned long long seg_max(unsigned long long v, uint32_t seg) {
  for (uint32_t d = 1; d < seg; d <<= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    if (o > v) v = o;
  }
  return v;
}

__device__ inline uint32_t seg_prefix(uint32_t v, uint32_t seg, uint32_t lane) {
  uint32_t inc = v;
  for (uint32_t d = 1; d < seg; d <<= 1) {
    const uint32_t y = __shfl_up(inc, d);
    if ((lane & (seg - 1)) >= d) inc += y;
  }
  return inc - v;
}

__global__ __launch_bounds__(kBlock) void k_groups_records(RowsSrc src, GroupsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool valid = i < a.n, ex = false;
  uint4 k = make_uint4(0u, 0u, 0u, 0u);
  if (valid) {
    k = src.key(i);
    if (k.x >= a.n_works || k.z >= a.n_script) valid = false;
  }
  if (__ballot(i < a.n && !valid) && lane == 0) atomicOr(&a.status[0], 1u);
  if (valid) ex = src.comb(i) <= 0.0;
  int first;
  unsigned long long kf;
  for (uint64_t todo = __ballot(valid); todo;) {
    const uint64_t m = same_key(todo, valid, k.x, &first, &kf);
    const uint32_t x = (uint32_t)__popcll(__ballot(ex) & m);
    if ((int)lane == first) {
      atomicAdd(&a.wstat[(size_t)kf * kWorkStats], (uint32_t)__popcll(m));
      if (x) atomicAdd(&a.wstat[(size_t)kf * kWorkStats + 1], x);
    }
    todo &= ~m;
  }
  if (!a.n_labels) return;                       // (wave-uniform)
  bool lab_ok = valid;
  unsigned long long key = 0;
  if (valid) {
    const uint32_t l = a.label_of[k.z];          // < n_labels: checked on the host
    key = (unsigned long long)k.x * a.n_labels + l;
  }
  for (uint64_t todo = __ballot(lab_ok); todo;) {
    const uint64_t m = same_key(todo, lab_ok, key, &first, &kf);
    const uint32_t x = (uint32_t)__popcll(__ballot(ex) & m);
    if ((int)lane == first) {
      atomicAdd(&a.wl[kf].x, (uint32_t)__popcll(m));
      if (x) atomicAdd(&a.wl[kf].y, x);
    }
    todo &= ~m;
  }
}

// one lane per run
__global__ __launch_bounds__(kBlock) void k_groups_runs(RowsSrc src, GroupsArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool keep = false;
  uint32_t w = 0, len = 0;
  if (r < a.n_runs) {
    const uint32_t h = a.heads[r], e = a.heads[r + 1];
    len = e - h;
    if (len >= a.min_words) {
      const uint4 k = src.key(h);
      const uint32_t o0 = k.z, o1 = src.key((uint64_t)e - 1).z;   // o0 <= o1: a run steps forward
      if (k.x < a.n_works && o1 < a.n_script && o0 <= o1) {
        keep = true;
        w = k.x;
        fs_cover_span(a.cov + (size_t)w * a.nk, 1, o0, o1);
      }
    }
  }
  int first;
  unsigned long long kf;
  for (uint64_t todo = __ballot(keep); todo;) {
    const uint64_t m = same_key(todo, keep, w, &first, &kf);
    const bool mine = (m >> lane) & 1;
    const uint32_t sum = wave_sum(mine ? len : 0u), top = wave_max(mine ? len : 0u);
    if ((int)lane == first) {
      uint32_t* s = a.wstat + (size_t)kf * kWorkStats;
      atomicAdd(&s[2], (uint32_t)__popcll(m));
      atomicAdd(&s[3], sum);
      atomicMax(&s[4], top);
    }
    todo &= ~m;
  }
}

// one lane per unit
__global__ __launch_bounds__(kBlock) void k_groups_stats(GroupsArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u >= a.n_units) return;
  const uint4 un = a.units[u];
  uint32_t works = 0, pworks = 0, words = 0, exact = 0, pas = 0, pwords = 0, longest = 0;
  for (uint32_t j = un.y; j < un.z; ++j) {
    const uint32_t* s = a.wstat + (size_t)a.members[j] * kWorkStats;
    works += s[0] != 0;
    pworks += s[2] != 0;
    words += s[0];
    exact += s[1];
    pas += s[2];
    pwords += s[3];
    longest = s[4] > longest ? s[4] : longest;
  }
  uint32_t* g = a.groups + (size_t)un.x * kGroupWords;
  if (works) atomicAdd(&g[G_WORKS], works);
  if (pworks) atomicAdd(&g[G_PWORKS], pworks);
  if (words) atomicAdd(&g[G_WORDS], words);
  if (exact) atomicAdd(&g[G_EXACT], exact);
  if (pas) atomicAdd(&g[G_PASSAGES], pas);
  if (pwords) atomicAdd(&g[G_PASSAGE_WORDS], pwords);
  if (longest) atomicMax(&g[G_LONGEST], longest);
}

// one lane per (unit, label)
__global__ __launch_bounds__(kBlock) void k_groups_labels(GroupsArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t u = idx / a.n_labels;
  const uint32_t l = (uint32_t)(idx % a.n_labels);
  if (u >= a.n_units) return;
  const uint4 un = a.units[u];
  uint32_t words = 0, exact = 0, works = 0;
  for (uint32_t j = un.y; j < un.z; ++j) {
    const uint2 v = a.wl[(size_t)a.members[j] * a.n_labels + l];
    words += v.x;
    exact += v.y;
    works += v.x != 0;
  }
  if (!words) return;
  const size_t at = (size_t)un.x * a.n_labels + l;
  atomicAdd(&a.glw[at], words);
  if (exact) atomicAdd(&a.glx[at], exact);
  atomicAdd(&a.glm[at], works);
}

// the column counts of 64 script words as bit planes: bit b of p[j] is bit j of word b's count
struct Planes {
  unsigned long long p[kPlanes];
  __device__ uint32_t at(uint32_t b) const {
    uint32_t d = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPlanes; ++j) d |= (uint32_t)((p[j] >> b) & 1) << j;
    return d;
  }
};

struct DepthRow {
  const uint32_t* row;          // the 64 counts
  __device__ uint32_t at(uint32_t b) const { return row[b]; }
};

// The figures of group g's words 64 k .. 64 k + 63, by every lane of the wave; `on`: this lane
// has such words.  any: depth >= 1, ge: depth >= min_works, key: the peak as in gpeak.
template <int kPlace, class Depth>
__device__ inline void words_tail(const GroupsArgs& a, bool on, uint32_t g, uint32_t k,
                                  unsigned long long any, unsigned long long ge,
                                  unsigned long long key, const Depth& depth) {
  const uint32_t lane = threadIdx.x & 63, seg = a.seg_k;
  const uint32_t rows = on ? (uint32_t)__popcll(ge) : 0u;
  if (!kPlace) {
    const uint32_t cov_s = seg_sum(on ? (uint32_t)__popcll(any) : 0u, seg);
    const uint32_t rows_s = seg_sum(rows, seg);
    const unsigned long long key_s = seg_max(on ? key : 0ull, seg);
    if (on && (lane & (seg - 1)) == 0) {
      uint32_t* gw = a.groups + (size_t)g * kGroupWords;
      if (cov_s) atomicAdd(&gw[G_COVERED], cov_s);
      if (rows_s) {
        atomicAdd(&gw[G_ROWS], rows_s);
        a.cbw[(size_t)g * a.nkb + (k >> 6)] = rows_s;
      }
      if (key_s) atomicMax(&a.gpeak[g], key_s);
    }
    return;
  }
  const uint32_t pre = seg_prefix(rows, seg, lane);
  if (!rows) return;
  unsigned long long at = a.woff[g] + pre;
  for (uint32_t j = 0; j < (k >> 6); ++j) at += a.cbw[(size_t)g * a.nkb + j];
  for (unsigned long long m = ge; m; m &= m - 1) {
    const uint32_t b = (uint32_t)__builtin_ctzll(m);
    reinterpret_cast<uint4*>(a.words)[at++] = make_uint4(g, k * 64 + b, depth.at(b), 0u);
  }
}

// one lane per (unit, 64 script words)
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_groups_depth(GroupsArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t u = idx / a.nkp;
  const uint32_t k = (uint32_t)(idx % a.nkp);
  bool on = u < a.n_units && k < a.nk;
  uint4 un = make_uint4(0u, 0u, 0u, FS_NONE);
  if (on) un = a.units[u];
  if (kPlace && un.w != FS_NONE) on = false;       // a split group: k_groups_big places it
  Planes pl;
#pragma unroll
  for (uint32_t j = 0; j < kPlanes; ++j) pl.p[j] = 0;
  if (on) {
#pragma unroll 4
    for (uint32_t j = un.y; j < un.z; ++j) {
      unsigned long long c = a.cov[(size_t)a.members[j] * a.nk + k];
#pragma unroll
      for (uint32_t q = 0; q < kPlanes; ++q) {       // at most kSplit = 2^kPlanes - 1 works
        const unsigned long long t = pl.p[q] & c;
        pl.p[q] ^= c;
        c = t;
      }
    }
  }
  unsigned long long any = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPlanes; ++j) any |= pl.p[j];
  if (on && un.w != FS_NONE) {                       // (count pass) one atomic per partial
    uint32_t* row = a.depth + ((size_t)un.w * a.nk + k) * 64;
    for (unsigned long long m = any; m; m &= m - 1) {
      const uint32_t b = (uint32_t)__builtin_ctzll(m);
      atomicAdd(&row[b], pl.at(b));
    }
    on = false;
  }
  // depth >= min_works, from the highest plane down; the peak and the first word that has it
  unsigned long long ge = 0, key = 0;
  if (on && any) {
    if (a.min_works <= kSplit) {
      unsigned long long gt = 0, eq = ~0ull;
#pragma unroll
      for (int j = kPlanes - 1; j >= 0; --j) {
        const unsigned long long tb = (a.min_works >> j) & 1 ? ~0ull : 0ull;
        gt |= eq & pl.p[j] & ~tb;
        eq &= ~(pl.p[j] ^ tb);
      }
      ge = gt | eq;
    }
    unsigned long long cand = any;
    uint32_t peak = 0;
#pragma unroll
    for (int j = kPlanes - 1; j >= 0; --j) {
      const unsigned long long t = cand & pl.p[j];
      if (t) {
        cand = t;
        peak |= 1u << j;
      }
    }
    key = ((unsigned long long)peak << 32) |
          (0xFFFFFFFFu - (k * 64 + (uint32_t)__builtin_ctzll(cand)));
  }
  words_tail<kPlace>(a, on, un.x, k, any, ge, key, pl);
}

// one lane per (split group, 64 script words)
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_groups_big(GroupsArgs a) {
  const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t s = idx / a.nkp;
  const uint32_t k = (uint32_t)(idx % a.nkp);
  const bool on = s < a.n_split && k < a.nk;
  unsigned long long any = 0, ge = 0, key = 0;
  uint32_t g = 0;
  DepthRow dr{a.depth};
  if (on) {
    g = a.split_group[s];
    dr.row = a.depth + ((size_t)s * a.nk + k) * 64;
    uint32_t peak = 0, at = 0;
    for (uint32_t b0 = 0; b0 < 64; b0 += 4) {
      const uint4 v = reinterpret_cast<const uint4*>(dr.row + b0)[0];
      const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        if (d[j]) any |= 1ull << (b0 + j);
        if (d[j] >= a.min_works) ge |= 1ull << (b0 + j);
        if (d[j] > peak) {
          peak = d[j];
          at = b0 + j;
        }
      }
    }
    if (peak) key = ((unsigned long long)peak << 32) | (0xFFFFFFFFu - (k * 64 + at));
  }
  words_tail<kPlace>(a, on, g, k, any, ge, key, dr);
}

// one lane per (group, label)
template <int kPlace>
__global__ __launch_bounds__(kBlock) void k_groups_cells(GroupsArgs a) {
  const uint32_t lane = threadIdx.x & 63, seg = a.seg_l;
  const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const uint64_t g = idx / a.nlp;
  const uint32_t l = (uint32_t)(idx % a.nlp);
  const bool on = g < a.n_groups && l < a.n_labels;
  const size_t at = on ? (size_t)g * a.n_labels + l : 0;
  const uint32_t words = on ? a.glw[at] : 0u;
  const uint32_t has = words != 0;
  if (!kPlace) {
    const uint32_t c = seg_sum(has, seg);
    const unsigned long long key =
        seg_max(has ? ((unsigned long long)words << 32) | (0xFFFFFFFFu - l) : 0ull, seg);
    if (on && c && (lane & (seg - 1)) == 0) {
      atomicAdd(&a.groups[(size_t)g * kGroupWords + G_CELLS], c);
      a.cbl[(size_t)g * a.nlb + (l >> 6)] = c;
      atomicMax(&a.gtop[g], key);
    }
    return;
  }
  const uint32_t pre = seg_prefix(has, seg, lane);
  if (!has) return;
  unsigned long long to = a.coff[g] + pre;
  for (uint32_t j = 0; j < (l >> 6); ++j) to += a.cbl[(size_t)g * a.nlb + j];
  fs_group_cell c;
  c.group = (uint32_t)g;
  c.label = l;
  c.n_words = words;
  c.n_exact = a.glx[at];
  c.n_works = a.glm[at];
  c.reserved = 0;
  a.cells[to] = c;
}

// one lane per group
__global__ __launch_bounds__(kBlock) void k_groups_finish(GroupsArgs a) {
  const uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  uint32_t* gw = a.groups + g * kGroupWords;
  const unsigned long long pk = a.gpeak[g], tp = a.gtop[g];
  gw[G_PEAK] = (uint32_t)(pk >> 32);
  gw[G_PEAK_FIRST] = pk ? 0xFFFFFFFFu - (uint32_t)pk : FS_NONE;
  gw[G_TOP] = tp ? 0xFFFFFFFFu - (uint32_t)tp : FS_NONE;
  gw[G_TOP_WORDS] = (uint32_t)(tp >> 32);
}

// exclusive scan of word `field` of every group into out, *total = sum (one workgroup)
__global__ __launch_bounds__(kScanBlock) void k_groups_scan(const uint32_t* groups, uint32_t field,
                                                            uint32_t nb, unsigned long long* out,
                                                            unsigned long long* total) {
  scan_array<unsigned long long, unsigned long long, kGroupWords>(groups + field, nb, out, total);
}

thread_local double t_ms[4];    // per-work tables, reduction by group, offsets, place pass

uint32_t seg_of(uint32_t items) {
  uint32_t s = 1;
  while (s < items && s < 64) s <<= 1;
  return s;
}

// the host part of one call: the checks and the group-major membership, nothing allocated on
// the device
struct GroupsPlan {
  std::vector<uint32_t> members, split_group;
  std::vector<uint4> units;
  uint32_t nk = 0;

  int make(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const uint64_t* mem_off,
           const uint32_t* mem_grp, uint32_t n_groups, const uint32_t* label_of,
           uint32_t n_labels, uint32_t min_words, uint32_t min_works) {
    if (min_words == 0 || min_works == 0) {
      fs_set_error("min_words and min_works must be at least 1");
      return FS_E_INVALID;
    }
    if ((n_works && !mem_off) || (n_labels && n_script && !label_of)) {
      fs_set_error("null argument");
      return FS_E_INVALID;
    }
    if (n_rows >= (1ull << 32)) {
      fs_set_error("%llu records: groups take fewer than 2^32", (unsigned long long)n_rows);
      return FS_E_UNSUPPORTED;
    }
    if (n_script > FS_WORKS_MAX_SCRIPT) {
      fs_set_error("n_script %u: groups take up to %u", n_script, FS_WORKS_MAX_SCRIPT);
      return FS_E_UNSUPPORTED;
    }
    if (n_works && mem_off[0] != 0) {
      fs_set_error("mem_off[0] is not 0");
      return FS_E_INVALID;
    }
    for (uint32_t w = 0; w < n_works; ++w)
      if (mem_off[w + 1] < mem_off[w]) {
        fs_set_error("mem_off[%u] > mem_off[%u]", w, w + 1);
        return FS_E_INVALID;
      }
    const uint64_t entries = n_works ? mem_off[n_works] : 0;
    if (entries && !mem_grp) {
      fs_set_error("null argument");
      return FS_E_INVALID;
    }
    if (entries > (uint64_t)n_works * n_groups) {      // (strictly ascending lists cannot)
      fs_set_error("more memberships than works x groups");
      return FS_E_INVALID;
    }
    for (uint32_t i = 0; n_labels && i < n_script; ++i)
      if (label_of[i] >= n_labels) {
        fs_set_error("label_of[%u] = %u with %u labels", i, label_of[i], n_labels);
        return FS_E_INVALID;
      }
    std::vector<uint64_t> start((size_t)n_groups + 1, 0);
    for (uint32_t w = 0; w < n_works; ++w)
      for (uint64_t j = mem_off[w]; j < mem_off[w + 1]; ++j) {
        const uint32_t g = mem_grp[j];
        if (g >= n_groups || (j > mem_off[w] && mem_grp[j - 1] >= g)) {
          fs_set_error("work %u: group %u outside the %u groups or not above the one before it",
                       w, g, n_groups);
          return FS_E_INVALID;
        }
        ++start[(size_t)g + 1];
      }
    uint64_t n_split = 0, n_units = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
      const uint64_t m = start[(size_t)g + 1];
      n_units += (m + kSplit - 1) / kSplit;
      n_split += m > kSplit;
      start[(size_t)g + 1] += start[g];
    }
    nk = (n_script + 63) / 64;
    const uint64_t nkb = (nk + 63) / 64, nlb = ((uint64_t)n_labels + 63) / 64;
    const uint64_t bytes = (uint64_t)n_works * nk * 8 + n_split * nk * 256 +
                           (uint64_t)n_works * n_labels * 8 + (uint64_t)n_groups * n_labels * 12 +
                           (uint64_t)n_groups * (nkb + nlb) * 4 + entries * 4 + n_units * 16;
    if (bytes > FS_GROUPS_MAX_BYTES) {
      fs_set_error("%u works in %u groups (%llu memberships) over %u script words and %u labels: "
                   "tables of %llu bytes, more than %u", n_works, n_groups,
                   (unsigned long long)entries, n_script, n_labels, (unsigned long long)bytes,
                   FS_GROUPS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    if (!n_rows || !n_groups) return FS_OK;            // nothing is built for these
    members.resize((size_t)entries);
    std::vector<uint64_t> cur(start.begin(), start.end() - 1);
    for (uint32_t w = 0; w < n_works; ++w)
      for (uint64_t j = mem_off[w]; j < mem_off[w + 1]; ++j) members[(size_t)cur[mem_grp[j]]++] = w;
    units.reserve((size_t)n_units);
    for (uint32_t g = 0; g < n_groups; ++g) {
      const uint64_t b = start[g], e = start[(size_t)g + 1];
      uint32_t row = FS_NONE;
      if (e - b > kSplit) {
        row = (uint32_t)split_group.size();
        split_group.push_back(g);
      }
      for (uint64_t s = b; s < e; s += kSplit)
        units.push_back(make_uint4(g, (uint32_t)s, (uint32_t)(s + kSplit < e ? s + kSplit : e), row));
    }
    return FS_OK;
  }
};

void groups_none(fs_group* groups, uint32_t n_groups) {
  fs_group none{};
  none.peak_first = FS_NONE;
  none.top_label = FS_NONE;
  for (uint32_t g = 0; g < n_groups; ++g) groups[g] = none;
}

// one call: count() through the groups and the two required counts, then write()
struct GroupsJob {
  DBuf<uint32_t> members, split_group, label_of, wstat, depth, glw, glx, glm, cbw, cbl, status;
  DBuf<uint4> units;
  DBuf<uint2> wl;
  DBuf<unsigned long long> cov, gpeak, gtop, woff, coff, totals;
  fs_runs* runs = nullptr;
  hipEvent_t ev[6] = {};
  GroupsArgs a{};
  uint64_t n_cells = 0, n_words = 0;
  ~GroupsJob() {
    if (runs) fs_runs_free(runs);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }

  int mark(int k, hipStream_t s) {
    if (!ev[k]) FS_HIP(hipEventCreate(&ev[k]));
    FS_HIP(hipEventRecord(ev[k], s));
    return FS_OK;
  }
  void elapsed(int k, int from, int to) {
    float ms = 0.f;
    t_ms[k] = hipEventElapsedTime(&ms, ev[from], ev[to]) == hipSuccess ? (double)ms : 0.0;
  }
  static dim3 grid(uint64_t lanes) { return dim3((uint32_t)((lanes + kBlock - 1) / kBlock)); }
  static bool fits(uint64_t lanes) { return (lanes + kBlock - 1) / kBlock <= 0x7FFFFFFFull; }

  // d_groups written, n_cells and n_words set (all on `s`, finished on return); n > 0 and
  // n_groups > 0
  int count(const fs_row* d_rows, const GroupsPlan& plan, uint32_t n, uint32_t n_works,
            uint32_t n_script, uint32_t n_groups, const uint32_t* label_of_host, uint32_t n_labels,
            uint32_t min_words, uint32_t max_gap, uint32_t min_works, fs_group* d_groups,
            hipStream_t s) {
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = plan.nk;
    a.n_groups = n_groups;
    a.n_labels = n_labels;
    a.min_words = min_words;
    a.min_works = min_works;
    a.seg_k = seg_of(a.nk);
    a.nkp = (a.nk + a.seg_k - 1) / a.seg_k * a.seg_k;
    a.nkb = (a.nk + 63) / 64;
    a.seg_l = seg_of(n_labels);
    a.nlp = (n_labels + a.seg_l - 1) / a.seg_l * a.seg_l;
    a.nlb = (n_labels + 63) / 64;
    a.n_units = (uint32_t)plan.units.size();
    a.n_split = (uint32_t)plan.split_group.size();
    a.groups = reinterpret_cast<uint32_t*>(d_groups);
    FS_TRY(fs_runs_find(d_rows, n, min_words, max_gap, s, &runs, &a.heads, &a.n_runs));
    if (!n_works || !n_script) return invalid();
    if (!fits((uint64_t)a.n_units * a.nkp) || !fits((uint64_t)a.n_units * n_labels) ||
        !fits((uint64_t)n_groups * a.nlp)) {
      fs_set_error("%u slabs of works: more lanes than a launch takes", a.n_units);
      return FS_E_UNSUPPORTED;
    }
    const size_t n_wl = (size_t)n_works * n_labels, n_gl = (size_t)n_groups * n_labels;
    const size_t n_cov = (size_t)n_works * a.nk, n_depth = (size_t)a.n_split * a.nk * 64;
    FS_TRY(members.upload(plan.members.data(), plan.members.size(), s));
    FS_TRY(units.upload(plan.units.data(), plan.units.size(), s));
    FS_TRY(split_group.upload(plan.split_group.data(), plan.split_group.size(), s));
    if (n_labels) FS_TRY(label_of.upload(label_of_host, n_script, s));
    FS_TRY(wstat.reserve((size_t)n_works * kWorkStats));
    FS_TRY(wl.reserve(n_wl));
    FS_TRY(cov.reserve(n_cov));
    FS_TRY(depth.reserve(n_depth));
    FS_TRY(glw.reserve(n_gl));
    FS_TRY(glx.reserve(n_gl));
    FS_TRY(glm.reserve(n_gl));
    FS_TRY(cbw.reserve((size_t)n_groups * a.nkb));
    FS_TRY(cbl.reserve((size_t)n_groups * a.nlb));
    FS_TRY(gpeak.reserve(n_groups));
    FS_TRY(gtop.reserve(n_groups));
    FS_TRY(woff.reserve(n_groups));
    FS_TRY(coff.reserve(n_groups));
    FS_TRY(totals.reserve(2));
    FS_TRY(status.reserve(4));
    FS_HIP(hipMemsetAsync(wstat.p, 0, (size_t)n_works * kWorkStats * sizeof(uint32_t), s));
    if (n_wl) FS_HIP(hipMemsetAsync(wl.p, 0, n_wl * sizeof(uint2), s));
    FS_HIP(hipMemsetAsync(cov.p, 0, n_cov * sizeof(unsigned long long), s));
    if (n_depth) FS_HIP(hipMemsetAsync(depth.p, 0, n_depth * sizeof(uint32_t), s));
    if (n_gl) {
      FS_HIP(hipMemsetAsync(glw.p, 0, n_gl * sizeof(uint32_t), s));
      FS_HIP(hipMemsetAsync(glx.p, 0, n_gl * sizeof(uint32_t), s));
      FS_HIP(hipMemsetAsync(glm.p, 0, n_gl * sizeof(uint32_t), s));
      FS_HIP(hipMemsetAsync(cbl.p, 0, (size_t)n_groups * a.nlb * sizeof(uint32_t), s));
    }
    FS_HIP(hipMemsetAsync(cbw.p, 0, (size_t)n_groups * a.nkb * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(gpeak.p, 0, (size_t)n_groups * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(gtop.p, 0, (size_t)n_groups * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(totals.p, 0, 2 * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(status.p, 0, 4 * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(d_groups, 0, (size_t)n_groups * sizeof(fs_group), s));
    a.label_of = n_labels ? label_of.p : nullptr;
    a.units = units.p;
    a.members = members.p;
    a.split_group = split_group.p;
    a.wstat = wstat.p;
    a.wl = wl.p;
    a.cov = cov.p;
    a.depth = depth.p;
    a.glw = glw.p;
    a.glx = glx.p;
    a.glm = glm.p;
    a.cbw = cbw.p;
    a.cbl = cbl.p;
    a.gpeak = gpeak.p;
    a.gtop = gtop.p;
    a.woff = woff.p;
    a.coff = coff.p;
    a.status = status.p;
    const dim3 blk(kBlock);
    FS_TRY(mark(0, s));
    const RowsSrc src{d_rows};
    hipLaunchKernelGGL(k_groups_records, grid(n), blk, 0, s, src, a);
    hipLaunchKernelGGL(k_groups_runs, grid(a.n_runs), blk, 0, s, src, a);
    FS_TRY(mark(1, s));
    if (a.n_units) {
      hipLaunchKernelGGL(k_groups_stats, grid(a.n_units), blk, 0, s, a);
      if (n_labels)
        hipLaunchKernelGGL(k_groups_labels, grid((uint64_t)a.n_units * n_labels), blk, 0, s, a);
      hipLaunchKernelGGL(k_groups_depth<0>, grid((uint64_t)a.n_units * a.nkp), blk, 0, s, a);
      if (a.n_split)
        hipLaunchKernelGGL(k_groups_big<0>, grid((uint64_t)a.n_split * a.nkp), blk, 0, s, a);
      if (n_labels)
        hipLaunchKernelGGL(k_groups_cells<0>, grid((uint64_t)n_groups * a.nlp), blk, 0, s, a);
    }
    FS_TRY(mark(2, s));
    hipLaunchKernelGGL(k_groups_finish, grid(n_groups), blk, 0, s, a);
    hipLaunchKernelGGL(k_groups_scan, dim3(1), dim3(kScanBlock), 0, s, a.groups, (uint32_t)G_CELLS,
                       n_groups, coff.p, totals.p);
    hipLaunchKernelGGL(k_groups_scan, dim3(1), dim3(kScanBlock), 0, s, a.groups, (uint32_t)G_ROWS,
                       n_groups, woff.p, totals.p + 1);
    FS_TRY(mark(3, s));
    FS_HIP(hipGetLastError());
    uint32_t st = 0;
    unsigned long long tot[2] = {0, 0};
    FS_HIP(hipMemcpyAsync(&st, status.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (st) return invalid();
    n_cells = tot[0];
    n_words = tot[1];
    elapsed(0, 0, 1);
    elapsed(1, 1, 2);
    elapsed(2, 2, 3);
    return FS_OK;
  }

  // the cells and the word rows (finished on return)
  int write(fs_group_cell* d_cells, fs_group_word* d_words, hipStream_t s) {
    if (!n_cells && !n_words) return FS_OK;
    a.cells = d_cells;
    a.words = d_words;
    const dim3 blk(kBlock);
    FS_TRY(mark(4, s));
    if (n_words) {
      hipLaunchKernelGGL(k_groups_depth<1>, grid((uint64_t)a.n_units * a.nkp), blk, 0, s, a);
      if (a.n_split)
        hipLaunchKernelGGL(k_groups_big<1>, grid((uint64_t)a.n_split * a.nkp), blk, 0, s, a);
    }
    if (n_cells)
      hipLaunchKernelGGL(k_groups_cells<1>, grid((uint64_t)a.n_groups * a.nlp), blk, 0, s, a);
    FS_TRY(mark(5, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    elapsed(3, 4, 5);
    return FS_OK;
  }

  static int invalid() {
    fs_set_error("a work >= n_works or an orig_ix >= n_script");
    return FS_E_INVALID;
  }
};

int groups_null(const void* groups, uint32_t n_groups, const void* cells, uint64_t cap_cells,
                const uint64_t* n_cells, const void* words, uint64_t cap_words,
                const uint64_t* n_words) {
  if (!n_cells || !n_words || (n_groups && !groups) || (cap_cells && !cells) ||
      (cap_words && !words)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_groups(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, const uint8_t* exact, uint64_t n_rows,
                         uint32_t n_works, uint32_t n_script, const uint64_t* mem_off,
                         const uint32_t* mem_grp, uint32_t n_groups, const uint32_t* label_of,
                         uint32_t n_labels, uint32_t min_words, uint32_t max_gap,
                         uint32_t min_works, fs_group* groups, fs_group_cell* cells,
                         uint64_t cap_cells, uint64_t* n_cells, fs_group_word* words,
                         uint64_t cap_words, uint64_t* n_words) {
  FS_TRY(groups_null(groups, n_groups, cells, cap_cells, n_cells, words, cap_words, n_words));
  for (double& t : t_ms) t = 0.0;
  GroupsPlan plan;
  FS_TRY(plan.make(n_rows, n_works, n_script, mem_off, mem_grp, n_groups, label_of, n_labels,
                   min_words, min_works));
  *n_cells = 0;
  *n_words = 0;
  if (!n_rows || !n_groups) {
    groups_none(groups, n_groups);
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix || !exact) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_group> d_groups;
  DBuf<fs_group_cell> d_cells;
  DBuf<fs_group_word> d_words;
  // the exact flags travel as comb: 0.0 where set, 1.0 where not
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n, nullptr, nullptr, exact));
  FS_TRY(d_groups.reserve(n_groups));
  GroupsJob job;
  FS_TRY(job.count(rows.p, plan, n, n_works, n_script, n_groups, label_of, n_labels, min_words,
                   max_gap, min_works, d_groups.p, nullptr));
  FS_TRY(copy_out(groups, d_groups, n_groups));
  *n_cells = job.n_cells;
  *n_words = job.n_words;
  if (job.n_cells > cap_cells || job.n_words > cap_words) return FS_E_CAPACITY;
  FS_TRY(d_cells.reserve(job.n_cells));
  FS_TRY(d_words.reserve(job.n_words));
  FS_TRY(job.write(d_cells.p, d_words.p, nullptr));
  if (job.n_cells) FS_TRY(copy_out(cells, d_cells, job.n_cells));
  if (job.n_words) FS_TRY(copy_out(words, d_words, job.n_words));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_groups_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                              uint32_t n_works, const uint64_t* mem_off, const uint32_t* mem_grp,
                              uint32_t n_groups, const uint32_t* label_of, uint32_t n_labels,
                              uint32_t min_words, uint32_t max_gap, uint32_t min_works,
                              fs_group* d_groups, fs_group_cell* d_cells, uint64_t cap_cells,
                              uint64_t* n_cells, fs_group_word* d_words, uint64_t cap_words,
                              uint64_t* n_words) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_TRY(groups_null(d_groups, n_groups, d_cells, cap_cells, n_cells, d_words, cap_words,
                     n_words));
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: groups take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  const uint32_t n_script = (uint32_t)ix->n_script;
  for (double& t : t_ms) t = 0.0;
  GroupsPlan plan;
  FS_TRY(plan.make(n_rows, n_works, n_script, mem_off, mem_grp, n_groups, label_of, n_labels,
                   min_words, min_works));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_groups & 15) ||
      ((uintptr_t)d_cells & 7) || ((uintptr_t)d_words & 15)) {
    fs_set_error("d_rows, d_groups and d_words must be 16-byte aligned device pointers, d_cells "
                 "8-byte");
    return FS_E_INVALID;
  }
  *n_cells = 0;
  *n_words = 0;
  if (!n_groups) return FS_OK;
  FS_ENTER(ix->device);
  if (!n_rows) {
    std::vector<fs_group> none(n_groups);
    groups_none(none.data(), n_groups);
    FS_HIP(hipMemcpyAsync(d_groups, none.data(), (size_t)n_groups * sizeof(fs_group),
                          hipMemcpyHostToDevice, ix->stream));
    FS_HIP(hipStreamSynchronize(ix->stream));
    return FS_OK;
  }
  GroupsJob job;
  FS_TRY(job.count(d_rows, plan, (uint32_t)n_rows, n_works, n_script, n_groups, label_of, n_labels,
                   min_words, max_gap, min_works, d_groups, ix->stream));
  *n_cells = job.n_cells;
  *n_words = job.n_words;
  if (job.n_cells > cap_cells || job.n_words > cap_words) return FS_E_CAPACITY;
  return job.write(d_cells, d_words, ix->stream);
}

extern "C" int fs_groups_times(double* ms) {
  return times_out(ms, t_ms, 4);
}
