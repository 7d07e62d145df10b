// fs_routes.hip -- `ao3.py routes`: sequences of stretches of the script that the fan works
// quote in that order (fs_routes, fs_routes_rows in include/fandom_search.h).  `transitions`
// relates the units one step at a time; this unit mines every route of 2 .. max_length units
// that at least min_all works follow, level by level, and one level more, which says of every
// listed route whether it is closed and how many frequent routes continue it.  It is bitmap
// sequence mining (SPAM) over 64-bit words: position space is the collapsed sequences of all
// works of two or more elements, one after the other; H and T mark the first and the last
// element of every work, M_u where the element is unit u, and B_P where an occurrence of route
// P ends.  B_(P + b) = step(B_P) & M_b, where step(X) is every position p behind a q of X, at
// most D away, with no head in (q, p]; works(P) is the works with a bit of B_P.
//
// Every output is an integer count, a minimum or an OR, and every place comes from a scanned
// count, so no schedule changes a byte.  Separate launches on one stream; no workgroup waits
// on another:
//   sequence         the checks, run heads and listed passages of fs_sequence.h, then
//   k_rt_kept        a lane per element: an element whose unit differs from the one in front
//                    (or that starts its work) stays; stayers counted per work
//   k_rt_flag        the stayers of works with two or more are positions; k_tr_scan numbers them
//   k_rt_positions   the unit and the work of every position
//   k_rt_marks       a wave per word of positions: H and T by ballot; works(u) as distinct
//                    (unit, work) keys of a set
//   k_rt_singles     F_1, k_rt_rows the M rows of its units
//  per level k -> k + 1:
//   k_rt_join        a lane per route of F_k: the routes that start with its last k - 1 units,
//                    a contiguous range found by binary search; its work items of kPiece
//   k_rt_edge        a workgroup per (route, slice): what the slice hands to the next one, for
//                    every carry-in it may get, and its last word
//   k_rt_step        the same grid: step(B_P) in place.  Any distance: a segmented fill inside
//                    the word in log steps under the propagate mask ~H, then the carry: a
//                    word generates (a bit behind its last head) or propagates (no head), the
//                    wave resolves its 64 words with one 64-bit add of the two ballots, the
//                    workgroup its waves through LDS, and the slice walks back over k_rt_edge's
//                    records to the last slice that decides.  Bounded: D <= 64, so a word
//                    needs the word in front only, 128 bits in log steps
//   k_rt_count       the hot pass, a workgroup per work item: the route's stepped row goes into
//                    LDS slice by slice with H and T; each wave takes extensions b in turn,
//                    ANDs with M_b and counts the works with a bit: fill(X) & T, with the same
//                    carry, kept per extension from chunk to chunk and slice to slice
//   k_tr_scan        the kept candidates numbered in candidate order: F_k+1 is sorted
//   k_rt_place       the kept candidates written as the next level, k_rt_bits their B rows,
//                    k_rt_first the work of their first bit
//   k_rt_mark        a lane per kept candidate: forward of its prefix, backward of its suffix,
//                    closed cleared on equal works
//  then
//   k_rt_tally       a lane per listed route: routes and longest of its units, the closed
//   k_rt_emit        the fs_route records
#include "fs_probe.h"
#include "fs_sequence.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSliceMax = kBlock;      // 64-bit words of a slice at most: one per thread
constexpr uint32_t kPerWave = 16;           // extensions a wave takes
constexpr uint32_t kPiece = 4 * kPerWave;   // extensions of a work item (tests: PIECE)
constexpr uint32_t kMaxLen = FS_ROUTES_MAX_LENGTH;

static_assert(sizeof(fs_route) == 64 && sizeof(fs_route_unit) == 16 &&
              sizeof(fs_route_level) == 24, "fs_routes");

typedef unsigned long long u64;

// F_k: n routes of k units each
struct RtLevel {
  uint32_t* items;              // [n][k]
  uint32_t* works;              // [n]
  uint32_t* first;              // [n] the smallest supporting work
  uint32_t* prefix;             // [n] works of the route without its last unit
  uint32_t* fwd;                // [n] frequent routes P + b
  uint32_t* bwd;                // [n] frequent routes a + P
  uint32_t* closed;             // [n]
  uint32_t* pre;                // [n] the route without its last unit, in the level below
  uint32_t* suf;                // [n] the route without its first unit, there too
  u64* bits;                    // [n][nw] B_P, then step(B_P)
  uint32_t n, k;
};

struct RtArgs {
  const u64* H;                 // [nw]
  const u64* T;
  const u64* M;                 // [|F_1|][nw]
  const uint32_t* row_of;       // [n_units] the M row of a frequent unit
  const uint32_t* work_at;      // [E]
  uint32_t E, nw;
  uint32_t D;                   // 0: any distance, else max_skip + 1
  uint32_t slice, n_slices;
  uint32_t min_all;
};

// ---- positions --------------------------------------------------------------------------

__device__ inline bool rt_stays(const SeqArgs& a, uint32_t p) {
  return p == 0 || a.work[p - 1] != a.work[p] || a.unit[p - 1] != a.unit[p];
}

__global__ __launch_bounds__(kBlock) void k_rt_kept(SeqArgs a, uint32_t* per_work) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < a.n_seq && rt_stays(a, p)) atomicAdd(&per_work[a.work[p]], 1u);
}

__global__ __launch_bounds__(kBlock) void k_rt_flag(SeqArgs a, const uint32_t* per_work,
                                                    uint32_t* flag) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < a.n_seq) flag[p] = rt_stays(a, p) && per_work[a.work[p]] >= 2 ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_rt_positions(SeqArgs a, const uint32_t* flag,
                                                         const uint32_t* pos, uint32_t* unit_at,
                                                         uint32_t* work_at) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n_seq || !flag[p]) return;
  unit_at[pos[p]] = a.unit[p];
  work_at[pos[p]] = a.work[p];
}

// a wave per word of positions
__global__ __launch_bounds__(kBlock) void k_rt_marks(uint32_t E, const uint32_t* unit_at,
                                                     const uint32_t* work_at, u64* H, u64* T,
                                                     u64* tab, uint64_t mask, uint32_t* uworks) {
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  const bool in = e < E;
  uint32_t w = 0;
  bool head = false, tail = false;
  if (in) {
    w = work_at[e];
    head = e == 0 || work_at[e - 1] != w;
    tail = e + 1 == E || work_at[e + 1] != w;
  }
  const uint64_t hb = __ballot(head), tb = __ballot(tail);
  if ((threadIdx.x & 63) == 0 && in) {
    H[e >> 6] = hb;
    T[e >> 6] = tb;
  }
  if (!in) return;
  const uint32_t u = unit_at[e];
  const u64 key = (u64)u << 32 | w;
  bool inserted;
  fs_probe_insert(tab, mask, fs_mix64(key), key, [key](u64 cur) { return cur == key; },
                  &inserted);
  if (inserted) atomicAdd(&uworks[u], 1u);
}

__global__ __launch_bounds__(kBlock) void k_rt_singles(const uint32_t* uworks, uint32_t n_units,
                                                       uint32_t min_all, uint32_t* flag) {
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
  if (u < n_units) flag[u] = uworks[u] >= min_all ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void k_rt_f1(const uint32_t* uworks, uint32_t n_units,
                                                  const uint32_t* flag, const uint32_t* row_of,
                                                  RtLevel f) {
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
  if (u >= n_units || !flag[u]) return;
  f.items[row_of[u]] = u;
  f.works[row_of[u]] = uworks[u];
}

__global__ __launch_bounds__(kBlock) void k_rt_rows(RtArgs a, const uint32_t* unit_at,
                                                    const uint32_t* flag, u64* M) {
  const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= a.E) return;
  const uint32_t u = unit_at[e];
  if (flag[u]) atomicOr(&M[(size_t)a.row_of[u] * a.nw + (e >> 6)], 1ull << (e & 63));
}

// ---- the bitwise rule -------------------------------------------------------------------

// x spread upwards through the positions `pro` lets it into (pro = ~H: not across a head)
__device__ inline uint64_t fill_up(uint64_t x, uint64_t pro) {
  x |= pro & (x << 1);
  pro &= pro << 1;
  x |= pro & (x << 2);
  pro &= pro << 2;
  x |= pro & (x << 4);
  pro &= pro << 4;
  x |= pro & (x << 8);
  pro &= pro << 8;
  x |= pro & (x << 16);
  pro &= pro << 16;
  x |= pro & (x << 32);
  return x;
}

// the positions of a word in front of its first head: where a carry-in lands
__device__ inline uint64_t below_head(uint64_t h) {
  return h ? (h & (0ull - h)) - 1 : ~0ull;
}

// what a word hands on: g, a bit at or behind its last head; p, no head and no bit
__device__ inline void word_gp(uint64_t x, uint64_t h, bool* g, bool* p) {
  if (!h) {
    *g = x != 0;
    *p = !*g;
  } else {
    *g = (x >> (63 - __clzll(h))) != 0;
    *p = false;
  }
}

// The carries of 64 words in lane order from the ballots of their g and p (disjoint): an add
// of G | P and G ripples a carry through the propagating words.  Returns the carry into every
// lane's word; *cout the carry out of the last.
__device__ inline uint64_t wave_carries(uint64_t G, uint64_t P, uint32_t cin, uint32_t* cout) {
  const uint64_t A = G | P, S = A + G + cin;
  *cout = (uint32_t)(((A & G) | (A & ~S)) >> 63);
  return S ^ A ^ G;
}

// step of word x (heads h) with the word in front (xp, hp), D <= 64: reach and the free way
// doubled in log steps, and put together along the bits of D
__device__ inline uint64_t step_bounded(uint64_t xp, uint64_t hp, uint64_t x, uint64_t h,
                                        uint32_t D) {
  typedef unsigned __int128 u128;
  const u128 X = (u128)x << 64 | xp, free1 = ~((u128)h << 64 | hp);
  u128 pw = (X << 1) & free1, pfree = free1;   // within 1 .. dp steps; no head in the dp up to p
  u128 r = 0, rfree = ~(u128)0;
  uint32_t d = 0, dp = 1;
  for (uint32_t bit = 0; bit < 7; ++bit) {
    if (D & (1u << bit)) {
      r |= (pw << d) & rfree;
      rfree &= pfree << d;
      d += dp;
    }
    pw |= (pw << dp) & pfree;
    pfree &= pfree << dp;
    dp <<= 1;
  }
  return (uint64_t)(r >> 64);
}

// the largest i < n with off[i] <= x, off ascending with off[0] = 0 and x < off[n]
__device__ inline uint32_t rt_owner(const u64* off, uint32_t n, u64 x) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- join -------------------------------------------------------------------------------

// the first k units of route x of `f` against key: -1, 0, 1
__device__ inline int rt_cmp(const RtLevel& f, uint64_t x, const uint32_t* key, uint32_t k) {
  const uint32_t* it = f.items + x * f.k;
  for (uint32_t t = 0; t < k; ++t) {
    if (it[t] != key[t]) return it[t] < key[t] ? -1 : 1;
  }
  return 0;
}

// One lane per route i of F_k: the routes that start with its last k - 1 units are
// lo[i] .. lo[i] + n_cand[i]; for k = 1 every other unit (n_cand = n - 1, no range).
__global__ __launch_bounds__(kBlock) void k_rt_join(RtLevel f, uint32_t* lo_out,
                                                    uint32_t* n_cand, uint32_t* n_item) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= f.n) return;
  uint32_t first = 0, n = f.n - 1;
  if (f.k > 1) {
    uint32_t key[kMaxLen + 1];
    for (uint32_t t = 0; t + 1 < f.k; ++t) key[t] = f.items[i * f.k + t + 1];
    uint32_t lo = 0, hi = f.n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rt_cmp(f, mid, key, f.k - 1) < 0) lo = mid + 1; else hi = mid;
    }
    first = lo;
    hi = f.n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (rt_cmp(f, mid, key, f.k - 1) <= 0) lo = mid + 1; else hi = mid;
    }
    n = lo - first;
  }
  lo_out[i] = first;
  n_cand[i] = n;
  n_item[i] = (n + kPiece - 1) / kPiece;
}

// one workgroup: out[j] = the sum of in[0 .. j), out[n] = *total = the sum of all
__global__ __launch_bounds__(kScanBlock) void k_rt_scan(const uint32_t* in, uint32_t n, u64* out,
                                                        u64* total) {
  __shared__ u64 s_total;
  scan_array<u64, u64>(in, n, out, &s_total);
  __syncthreads();
  if (threadIdx.x == 0) out[n] = *total = s_total;
}

// extension e of route i of F_k: the route of F_k it is joined with
__device__ inline uint32_t rt_partner(const RtLevel& f, const uint32_t* lo, uint32_t i,
                                      uint32_t e) {
  if (f.k == 1) return e < i ? e : e + 1;
  return lo[i] + e;
}

__global__ __launch_bounds__(kBlock) void k_rt_cands(RtLevel f, const u64* off, uint64_t n_cands,
                                                     uint32_t* parent) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c < n_cands) parent[c] = rt_owner(off, f.n, c);
}

// ---- step -------------------------------------------------------------------------------

// blockIdx.x = route * n_slices + slice, a thread per word of the slice.  The workgroup's
// carry-out under carry-in 0 and under 1 (bits 0 and 1 of sum), and its last word.
__global__ __launch_bounds__(kBlock) void k_rt_edge(RtArgs a, RtLevel f, uint32_t* sum,
                                                    u64* edge) {
  __shared__ uint32_t s_c[2][kBlock / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x / a.n_slices, sl = blockIdx.x % a.n_slices;
  const uint32_t w = sl * a.slice + threadIdx.x;
  const bool in = threadIdx.x < a.slice && w < a.nw;
  uint64_t x = 0, h = 0;
  if (in) {
    x = f.bits[(size_t)r * a.nw + w];
    h = a.H[w];
    if (threadIdx.x + 1 == a.slice || w + 1 == a.nw) edge[blockIdx.x] = x;
  }
  bool g, p;
  word_gp(x, h, &g, &p);                               // (a word outside: propagates)
  const uint64_t G = __ballot(g), P = __ballot(p);
  uint32_t c0, c1;
  wave_carries(G, P, 0u, &c0);
  wave_carries(G, P, 1u, &c1);
  if (lane == 0) {
    s_c[0][wave] = c0;
    s_c[1][wave] = c1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t z = 0, o = 1;
    for (uint32_t v = 0; v < kBlock / 64; ++v) {
      z = s_c[z][v];
      o = s_c[o][v];
    }
    sum[blockIdx.x] = z | o << 1;
  }
}

// the same grid: step(B_P) in place of B_P
__global__ __launch_bounds__(kBlock) void k_rt_step(RtArgs a, RtLevel f, const uint32_t* sum,
                                                    const u64* edge) {
  __shared__ uint32_t s_c[2][kBlock / 64];
  __shared__ uint32_t s_in;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t r = blockIdx.x / a.n_slices, sl = blockIdx.x % a.n_slices;
  const uint32_t w = sl * a.slice + threadIdx.x;
  const bool in = threadIdx.x < a.slice && w < a.nw;
  u64* row = f.bits + (size_t)r * a.nw;
  uint64_t x = 0, h = 0, y = 0;
  if (in) {
    x = row[w];
    h = a.H[w];
  }
  if (a.D) {                                           // (uniform)
    uint64_t xp = 0, hp = 0;
    if (in && w) {
      xp = threadIdx.x ? row[w - 1] : edge[blockIdx.x - 1];
      hp = a.H[w - 1];
    }
    y = step_bounded(xp, hp, x, h, a.D);
    __syncthreads();                                   // every word in front is read
    if (in) row[w] = y;
    return;
  }
  if (threadIdx.x == 0) {
    // the carry into the slice: back to the last slice that decides whatever it is handed
    uint32_t c = 0;
    for (uint32_t s = sl; s > 0; --s) {
      const uint32_t v = sum[blockIdx.x - (sl - s) - 1];
      if (v != 2u) {                                   // (2: out 0 under 0, 1 under 1)
        c = v & 1u;
        break;
      }
    }
    s_in = c;
  }
  bool g, p;
  word_gp(x, h, &g, &p);
  const uint64_t G = __ballot(g), P = __ballot(p);
  uint32_t c0, c1;
  wave_carries(G, P, 0u, &c0);
  wave_carries(G, P, 1u, &c1);
  if (lane == 0) {
    s_c[0][wave] = c0;
    s_c[1][wave] = c1;
  }
  __syncthreads();
  uint32_t c = s_in;
  for (uint32_t v = 0; v < wave; ++v) c = s_c[c][v];
  uint32_t out;
  const uint64_t C = wave_carries(G, P, c, &out);
  y = fill_up((x << 1) & ~h, ~h);
  if ((C >> lane) & 1) y |= below_head(h);
  if (in) row[w] = y;
}

// ---- count ------------------------------------------------------------------------------

// blockIdx.x = a work item: piece p of the extensions of route i.
__global__ __launch_bounds__(kBlock) void k_rt_count(RtArgs a, RtLevel f, const uint32_t* lo,
                                                     const u64* cand_off, const u64* item_off,
                                                     uint32_t* count, uint32_t* keep) {
  __shared__ u64 s_par[kSliceMax];
  __shared__ u64 s_h[kSliceMax];
  __shared__ u64 s_t[kSliceMax];
  __shared__ uint32_t s_ext[kPiece];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t i = rt_owner(item_off, f.n, blockIdx.x);
  const u64 c0 = cand_off[i];
  const uint32_t n_ext = (uint32_t)(cand_off[i + 1] - c0);
  const uint32_t e0 = (uint32_t)(blockIdx.x - item_off[i]) * kPiece;
  if (threadIdx.x < kPiece) {
    const uint32_t e = e0 + threadIdx.x;
    uint32_t x = FS_NONE;
    if (e < n_ext) {
      const uint32_t j = rt_partner(f, lo, i, e);
      x = a.row_of[f.items[(uint64_t)j * f.k + f.k - 1]];
    }
    s_ext[threadIdx.x] = x;
  }
  uint32_t acc[kPerWave] = {};
  uint32_t carry = 0;                                  // bit t: extension t's open work has a bit
  const uint32_t nw = a.nw;
  const u64* par = f.bits + (size_t)i * nw;
  for (uint32_t k0 = 0; k0 < nw; k0 += a.slice) {
    __syncthreads();                                   // s_ext; the slice before
    const uint32_t here = nw - k0 < a.slice ? nw - k0 : a.slice;
    if (threadIdx.x < here) {
      s_par[threadIdx.x] = par[k0 + threadIdx.x];
      s_h[threadIdx.x] = a.H[k0 + threadIdx.x];
      s_t[threadIdx.x] = a.T[k0 + threadIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t t = 0; t < kPerWave; ++t) {
      const uint32_t m = s_ext[wave * kPerWave + t];
      if (m == FS_NONE) continue;                      // (wave-uniform)
      const u64* mrow = a.M + (size_t)m * nw + k0;
      uint32_t c = (carry >> t) & 1u;
      for (uint32_t q = 0; q < here; q += 64) {
        const uint32_t w = q + lane;
        uint64_t x = 0, h = 0, tl = 0;
        if (w < here) {
          x = s_par[w] & mrow[w];
          h = s_h[w];
          tl = s_t[w];
        }
        bool g, p;
        word_gp(x, h, &g, &p);
        const uint64_t C = wave_carries(__ballot(g), __ballot(p), c, &c);
        uint64_t fl = fill_up(x, ~h);
        if ((C >> lane) & 1) fl |= below_head(h);
        acc[t] += (uint32_t)__popcll(fl & tl);
      }
      carry = (carry & ~(1u << t)) | c << t;
    }
  }
#pragma unroll
  for (uint32_t t = 0; t < kPerWave; ++t) {
    const uint32_t e = e0 + wave * kPerWave + t;
    if (e >= n_ext) break;                             // (wave-uniform)
    const uint32_t n = wave_sum(acc[t]);
    if (lane == 0) {
      count[c0 + e] = n;
      keep[c0 + e] = n >= a.min_all ? 1u : 0u;
    }
  }
}

// ---- place, mark, records ---------------------------------------------------------------

// one lane per candidate: a kept one becomes route pos[c] of F_k+1
__global__ __launch_bounds__(kBlock) void k_rt_place(RtLevel f, RtLevel g, const uint32_t* lo,
                                                     const u64* cand_off, uint64_t n_cands,
                                                     const uint32_t* parent,
                                                     const uint32_t* count, const uint32_t* keep,
                                                     const uint32_t* pos) {
  const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cands || !keep[c]) return;
  const uint32_t i = parent[c], j = rt_partner(f, lo, i, (uint32_t)(c - cand_off[i]));
  const uint64_t p = pos[c];
  for (uint32_t t = 0; t < f.k; ++t) g.items[p * g.k + t] = f.items[(uint64_t)i * f.k + t];
  g.items[p * g.k + f.k] = f.items[(uint64_t)j * f.k + f.k - 1];
  g.works[p] = count[c];
  g.first[p] = FS_NONE;
  g.prefix[p] = f.works[i];
  g.fwd[p] = 0u;
  g.bwd[p] = 0u;
  g.closed[p] = 1u;
  g.pre[p] = i;
  g.suf[p] = j;
}

// one lane per word of the new rows: B_(P + b) = step(B_P) & M_b
__global__ __launch_bounds__(kBlock) void k_rt_bits(RtArgs a, RtLevel f, RtLevel g) {
  const uint64_t x = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (x >= (uint64_t)g.n * a.nw) return;
  const uint64_t s = x / a.nw;
  const uint32_t w = (uint32_t)(x % a.nw);
  const uint32_t b = g.items[s * g.k + g.k - 1];
  g.bits[x] = f.bits[(size_t)g.pre[s] * a.nw + w] & a.M[(size_t)a.row_of[b] * a.nw + w];
}

// One lane per route: its first bit lies in the first work that follows it.  A frequent
// route has works >= 1, so it is found.
__global__ __launch_bounds__(kBlock) void k_rt_first(RtArgs a, RtLevel g) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= g.n) return;
  const u64* row = g.bits + s * a.nw;
  for (uint32_t w = 0; w < a.nw; ++w) {
    if (row[w]) {
      g.first[s] = a.work_at[w * 64 + (uint32_t)__builtin_ctzll(row[w])];
      return;
    }
  }
}

// one lane per route of g = F_k+1
__global__ __launch_bounds__(kBlock) void k_rt_mark(RtLevel f, RtLevel g) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= g.n) return;
  const uint32_t i = g.pre[s], j = g.suf[s], n = g.works[s];
  atomicAdd(&f.fwd[i], 1u);
  atomicAdd(&f.bwd[j], 1u);
  if (f.works[i] == n) f.closed[i] = 0u;               // (every writer writes 0)
  if (f.works[j] == n) f.closed[j] = 0u;
}

// one lane per route of a listed level: *n_closed the closed routes of the level
__global__ __launch_bounds__(kBlock) void k_rt_tally(RtLevel f, fs_route_unit* units,
                                                     uint32_t* n_closed) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool in = s < f.n;
  if (in) {
    const uint32_t* it = f.items + s * f.k;
    for (uint32_t t = 0; t < f.k; ++t) {
      bool seen = false;                               // a unit that returns counts once
      for (uint32_t v = 0; v < t; ++v) seen |= it[v] == it[t];
      if (seen) continue;
      atomicAdd(&units[it[t]].routes, 1u);
      atomicMax(&units[it[t]].longest, f.k);
    }
  }
  const uint64_t mc = __ballot(in && f.closed[s]);
  if ((threadIdx.x & 63) == 0 && mc) atomicAdd(n_closed, (uint32_t)__popcll(mc));
}

// one lane per unit
__global__ __launch_bounds__(kBlock) void k_rt_units(const uint32_t* uworks, fs_route_unit* units,
                                                     uint32_t n_units) {
  const uint64_t u = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (u < n_units)
    reinterpret_cast<uint4*>(units)[u] = make_uint4(uworks ? uworks[u] : 0u, 0u, 0u, 0u);
}

// one lane per route: record base + s
__global__ __launch_bounds__(kBlock) void k_rt_emit(RtLevel f, fs_route* out, uint64_t base) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (s >= f.n) return;
  uint32_t u[kMaxLen];
  for (uint32_t t = 0; t < kMaxLen; ++t) u[t] = t < f.k ? f.items[s * f.k + t] : FS_NONE;
  uint4* o = reinterpret_cast<uint4*>(out + base + s);
  o[0] = make_uint4(u[0], u[1], u[2], u[3]);
  o[1] = make_uint4(u[4], u[5], u[6], u[7]);
  o[2] = make_uint4(f.k, f.works[s], f.first[s], f.prefix[s]);
  o[3] = make_uint4(f.fwd[s], f.bwd[s], f.closed[s], 0u);
}

// ---- host -------------------------------------------------------------------------------

constexpr int kTimes = FS_ROUTES_TIMES;
thread_local double t_ms[kTimes];   // fs_routes_times in include/fandom_search.h

struct LevelBufs {
  DBuf<uint32_t> items, figures;    // figures: works, first, prefix, fwd, bwd, closed, pre, suf
  DBuf<u64> bits;
  int reserve(uint64_t n, uint32_t k) {
    FS_TRY(items.reserve(n * k));
    FS_TRY(figures.reserve(n * 8));
    return FS_OK;
  }
  RtLevel view(uint64_t n, uint32_t k) {
    uint32_t* p = figures.p;
    return RtLevel{items.p, p,         p + n,     p + 2 * n, p + 3 * n, p + 4 * n,
                   p + 5 * n, p + 6 * n, p + 7 * n, bits.p,   (uint32_t)n, k};
  }
};

// one call: mine() through the units, the levels and the number of routes, then write()
struct RtJob {
  SeqJob sq;
  DBuf<uint32_t> per_work, flag, pos, unit_at, work_at, uworks, single, row_of, lo, n_cand,
      n_item, parent, count, keep, kpos, sum, stats;
  DBuf<u64> H, T, M, tab, cand_off, item_off, totals, edge;
  DBuf<fs_route_unit> units;        // the caller's are written when nothing can refuse any more
  LevelBufs lv[kMaxLen + 2];        // by length
  RtLevel f[kMaxLen + 2] = {};
  Clock<64> clk;
  SeqArgs q{};
  RtArgs a{};
  uint32_t max_length = 0, n_units = 0;
  uint64_t n_routes = 0, max_sets = 0, bytes = 0, scratch = 0;
  fs_route_level levels[kMaxLen] = {};       // lengths 2 .. max_length + 1

  void blank_levels() {
    for (uint32_t k = 2; k <= max_length + 1; ++k)
      levels[k - 2] = fs_route_level{k, 0u, 0ull, k > max_length ? FS_NONE : 0u, 0u};
  }

  int none(fs_route_unit* d_units, hipStream_t s) {
    if (n_units)
      hipLaunchKernelGGL(k_rt_units, dim3(blocks_of(n_units, kBlock)), dim3(kBlock), 0, s,
                         (const uint32_t*)nullptr, d_units, n_units);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    return FS_OK;
  }

  // what the tables of a call hold, against FS_ROUTES_MAX_BYTES
  // (`more` stays for the call, `now` is scratch that the next level uses again)
  int room(uint64_t more, uint64_t now, uint32_t length, const char* what) {
    bytes += more;
    if (now > scratch) scratch = now;
    if (bytes + scratch > FS_ROUTES_MAX_BYTES) {
      fs_set_error("routes: the position tables, the bitmap rows of two levels, the level "
                   "lists and the candidate buffers come to more than %u bytes at %s of "
                   "length %u; raise --min-all or lower --max-length", FS_ROUTES_MAX_BYTES,
                   what, length);
      return FS_E_UNSUPPORTED;
    }
    return FS_OK;
  }

  int too_many(uint32_t length, u64 n) {
    fs_set_error("routes: level %u has %llu candidate routes, more than %llu "
                 "(FS_ROUTES_MAX_SETS); raise --min-all or lower --max-length", length, n,
                 (u64)max_sets);
    return FS_E_UNSUPPORTED;
  }

  // d_units written, levels and n_routes set (all on `s`, finished on return)
  int mine(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
           const uint32_t* d_unit_of, uint32_t nu, uint32_t min_words, uint32_t max_gap,
           uint32_t max_skip, uint32_t min_all, uint32_t l_max, fs_route_unit* d_units,
           hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    max_length = l_max;
    n_units = nu;
    blank_levels();
    q.n = n;
    q.n_works = n_works;
    q.n_script = n_script;
    q.unit_of = d_unit_of;
    q.n_units = nu;
    q.min_words = min_words;
    if (!n || !nu) return none(d_units, s);
    max_sets = env_u32("FS_ROUTES_MAX_SETS", FS_ROUTES_MAX_SETS, 1u << 26);
    a.slice = env_u32("FS_ROUTES_SLICE_WORDS", kSliceMax, kSliceMax);
    if (!a.slice) a.slice = 1;
    a.D = max_skip == FS_NONE ? 0u : max_skip + 1;
    a.min_all = min_all;
    const dim3 blk(kBlock);
    FS_TRY(clk.mark(0, s));
    FS_TRY(sq.list(d_rows, q, max_gap, s));
    if (!q.n_seq) return none(d_units, s);

    // the positions
    const uint32_t seq_blocks = blocks_of(q.n_seq, kBlock);
    FS_TRY(per_work.reserve(n_works));
    FS_TRY(flag.reserve(q.n_seq));
    FS_TRY(pos.reserve(q.n_seq));
    FS_TRY(totals.reserve(2));
    FS_TRY(stats.reserve(kMaxLen + 2));
    FS_HIP(hipMemsetAsync(per_work.p, 0, (size_t)n_works * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(stats.p, 0, (kMaxLen + 2) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_rt_kept, dim3(seq_blocks), blk, 0, s, q, per_work.p);
    hipLaunchKernelGGL(k_rt_flag, dim3(seq_blocks), blk, 0, s, q, (const uint32_t*)per_work.p,
                       flag.p);
    hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(kScanBlock), 0, s, (const uint32_t*)flag.p,
                       pos.p, q.n_seq, totals.p, (uint32_t*)nullptr);
    FS_HIP(hipGetLastError());
    u64 tot[2] = {0, 0};
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot[0], hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    a.E = (uint32_t)tot[0];
    if (!a.E) return none(d_units, s);
    a.nw = (a.E + 63) / 64;
    a.n_slices = (a.nw + a.slice - 1) / a.slice;
    const uint64_t slots = fs_probe_slots(a.E);
    FS_TRY(room((uint64_t)a.E * 8 + (uint64_t)a.nw * 16 + slots * 8 + (uint64_t)nu * 12, 0, 1,
                "the positions"));
    FS_TRY(unit_at.reserve(a.E));
    FS_TRY(work_at.reserve(a.E));
    FS_TRY(H.reserve(a.nw));
    FS_TRY(T.reserve(a.nw));
    FS_TRY(tab.reserve(slots));
    FS_TRY(uworks.reserve(nu));
    FS_TRY(single.reserve(nu));
    FS_TRY(row_of.reserve(nu));
    FS_TRY(units.reserve(nu));
    FS_HIP(hipMemsetAsync(tab.p, 0xFF, slots * sizeof(u64), s));
    FS_HIP(hipMemsetAsync(uworks.p, 0, (size_t)nu * sizeof(uint32_t), s));
    a.H = H.p;
    a.T = T.p;
    a.row_of = row_of.p;
    a.work_at = work_at.p;
    hipLaunchKernelGGL(k_rt_positions, dim3(seq_blocks), blk, 0, s, q, (const uint32_t*)flag.p,
                       (const uint32_t*)pos.p, unit_at.p, work_at.p);
    hipLaunchKernelGGL(k_rt_marks, dim3(blocks_of((uint64_t)a.nw * 64, kBlock)), blk, 0, s, a.E,
                       (const uint32_t*)unit_at.p, (const uint32_t*)work_at.p, H.p, T.p, tab.p,
                       slots - 1, uworks.p);
    hipLaunchKernelGGL(k_rt_singles, dim3(blocks_of(nu, kBlock)), blk, 0, s,
                       (const uint32_t*)uworks.p, nu, min_all, single.p);
    hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(kScanBlock), 0, s, (const uint32_t*)single.p,
                       row_of.p, nu, totals.p, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_rt_units, dim3(blocks_of(nu, kBlock)), blk, 0, s,
                       (const uint32_t*)uworks.p, units.p, nu);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot[0], hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    const uint64_t n1 = tot[0];
    f[1] = RtLevel{};
    f[1].k = 1;
    if (n1) {
      // M, and F_1 with a copy of it as its rows
      FS_TRY(room(n1 * a.nw * 8, n1 * (a.nw * 8 + 36), 1, "the rows of the units"));
      FS_TRY(M.reserve(n1 * a.nw));
      FS_TRY(lv[1].reserve(n1, 1));
      FS_TRY(lv[1].bits.reserve(n1 * a.nw));
      f[1] = lv[1].view(n1, 1);
      a.M = M.p;
      FS_HIP(hipMemsetAsync(M.p, 0, n1 * a.nw * sizeof(u64), s));
      hipLaunchKernelGGL(k_rt_rows, dim3(blocks_of(a.E, kBlock)), blk, 0, s, a,
                         (const uint32_t*)unit_at.p, (const uint32_t*)single.p, M.p);
      hipLaunchKernelGGL(k_rt_f1, dim3(blocks_of(nu, kBlock)), blk, 0, s,
                         (const uint32_t*)uworks.p, nu, (const uint32_t*)single.p,
                         (const uint32_t*)row_of.p, f[1]);
      FS_HIP(hipGetLastError());
      FS_HIP(hipMemcpyAsync(lv[1].bits.p, M.p, n1 * a.nw * sizeof(u64), hipMemcpyDeviceToDevice,
                            s));
    }
    FS_TRY(clk.mark(1, s));
    FS_HIP(hipStreamSynchronize(s));
    t_ms[0] = clk.elapsed(0, 1);
    for (uint32_t k = 1; k <= max_length; ++k) FS_TRY(level(k, s));
    FS_TRY(clk.mark(2, s));
    for (uint32_t k = 2; k <= max_length; ++k) {
      if (!f[k].n) continue;
      hipLaunchKernelGGL(k_rt_tally, dim3(blocks_of(f[k].n, kBlock)), blk, 0, s, f[k], units.p,
                         stats.p + k);
      n_routes += f[k].n;
    }
    FS_TRY(clk.mark(3, s));
    FS_HIP(hipGetLastError());
    uint32_t st[kMaxLen + 2];
    FS_HIP(hipMemcpyAsync(st, stats.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(d_units, units.p, (size_t)nu * sizeof(fs_route_unit),
                          hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    for (uint32_t k = 2; k <= max_length; ++k) levels[k - 2].closed = st[k];
    t_ms[kTimes - 2] = clk.elapsed(2, 3);
    return FS_OK;
  }

  // F_k+1 from F_k, and what it says about F_k
  int level(uint32_t k, hipStream_t s) {
    const uint32_t n = f[k].n;
    f[k + 1] = RtLevel{};
    f[k + 1].k = k + 1;
    if (k >= 2) lv[k - 1].bits.release();                // two adjacent levels of rows at a time
    if (!n || (k == 1 && n < 2)) return FS_OK;
    const dim3 blk(kBlock);
    const int m0 = 4 + (int)(k - 1) * 6;                 // marks of this level
    double* t = t_ms + 1 + (k - 1) * 5;
    const uint64_t row_bytes = (uint64_t)a.nw * 8;
    FS_TRY(room(0, (uint64_t)n * (row_bytes + 28), k + 1, "the join"));
    FS_TRY(lo.reserve(n));
    FS_TRY(n_cand.reserve(n));
    FS_TRY(n_item.reserve(n));
    FS_TRY(cand_off.reserve((size_t)n + 1));
    FS_TRY(item_off.reserve((size_t)n + 1));
    FS_TRY(clk.mark(m0, s));
    hipLaunchKernelGGL(k_rt_join, dim3(blocks_of(n, kBlock)), blk, 0, s, f[k], lo.p, n_cand.p,
                       n_item.p);
    hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(kScanBlock), 0, s, (const uint32_t*)n_cand.p,
                       n, cand_off.p, totals.p);
    hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(kScanBlock), 0, s, (const uint32_t*)n_item.p,
                       n, item_off.p, totals.p + 1);
    FS_HIP(hipGetLastError());
    u64 tot[2] = {0, 0};
    FS_HIP(hipMemcpyAsync(tot, totals.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    levels[k - 1].candidates = tot[0];
    if (tot[0] > max_sets) return too_many(k + 1, tot[0]);
    if (!tot[0]) return FS_OK;
    const uint64_t grid = (uint64_t)n * a.n_slices;
    if (grid > 0x7FFFFFFFull || tot[1] > 0x7FFFFFFFull) {
      fs_set_error("routes: level %u has more slices of rows than a launch takes; raise "
                   "--min-all or lower --max-length", k + 1);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(room(0, (uint64_t)n * (row_bytes + 28) + grid * 12 + tot[0] * 16, k + 1,
                "the candidates"));
    FS_TRY(parent.reserve(tot[0]));
    FS_TRY(count.reserve(tot[0]));
    FS_TRY(keep.reserve(tot[0]));
    FS_TRY(kpos.reserve(tot[0]));
    FS_TRY(sum.reserve(grid));
    FS_TRY(edge.reserve(grid));
    hipLaunchKernelGGL(k_rt_cands, dim3(blocks_of(tot[0], kBlock)), blk, 0, s, f[k],
                       (const u64*)cand_off.p, (uint64_t)tot[0], parent.p);
    FS_TRY(clk.mark(m0 + 1, s));
    hipLaunchKernelGGL(k_rt_edge, dim3((uint32_t)grid), blk, 0, s, a, f[k], sum.p, edge.p);
    hipLaunchKernelGGL(k_rt_step, dim3((uint32_t)grid), blk, 0, s, a, f[k],
                       (const uint32_t*)sum.p, (const u64*)edge.p);
    FS_TRY(clk.mark(m0 + 2, s));
    hipLaunchKernelGGL(k_rt_count, dim3((uint32_t)tot[1]), blk, 0, s, a, f[k],
                       (const uint32_t*)lo.p, (const u64*)cand_off.p, (const u64*)item_off.p,
                       count.p, keep.p);
    FS_TRY(clk.mark(m0 + 3, s));
    hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(kScanBlock), 0, s, (const uint32_t*)keep.p,
                       kpos.p, (uint32_t)tot[0], totals.p, (uint32_t*)nullptr);
    FS_HIP(hipGetLastError());
    u64 kept = 0;
    FS_HIP(hipMemcpyAsync(&kept, totals.p, sizeof kept, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    levels[k - 1].frequent = (uint32_t)kept;
    t[0] = clk.elapsed(m0, m0 + 1);
    t[1] = clk.elapsed(m0 + 1, m0 + 2);
    t[2] = clk.elapsed(m0 + 2, m0 + 3);
    if (!kept) return FS_OK;
    const bool listed = k + 1 <= max_length;             // and the parents of a level more
    FS_TRY(room(kept * (k + 1 + 8) * 4, (uint64_t)n * (row_bytes + 28) + grid * 12 +
                tot[0] * 16 + (listed ? kept * row_bytes : 0), k + 1, "the list"));
    FS_TRY(lv[k + 1].reserve(kept, k + 1));
    if (listed) FS_TRY(lv[k + 1].bits.reserve(kept * a.nw));
    f[k + 1] = lv[k + 1].view(kept, k + 1);
    hipLaunchKernelGGL(k_rt_place, dim3(blocks_of(tot[0], kBlock)), blk, 0, s, f[k], f[k + 1],
                       (const uint32_t*)lo.p, (const u64*)cand_off.p, (uint64_t)tot[0],
                       (const uint32_t*)parent.p, (const uint32_t*)count.p,
                       (const uint32_t*)keep.p, (const uint32_t*)kpos.p);
    if (listed) {
      hipLaunchKernelGGL(k_rt_bits, dim3(blocks_of(kept * a.nw, kBlock)), blk, 0, s, a, f[k],
                         f[k + 1]);
      hipLaunchKernelGGL(k_rt_first, dim3(blocks_of(kept, kBlock)), blk, 0, s, a, f[k + 1]);
    }
    FS_TRY(clk.mark(m0 + 4, s));
    if (k >= 2)
      hipLaunchKernelGGL(k_rt_mark, dim3(blocks_of(kept, kBlock)), blk, 0, s, f[k], f[k + 1]);
    FS_TRY(clk.mark(m0 + 5, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t[3] = clk.elapsed(m0 + 3, m0 + 4);
    t[4] = clk.elapsed(m0 + 4, m0 + 5);
    return FS_OK;
  }

  // the n_routes records into d_routes (finished on return)
  int write(fs_route* d_routes, hipStream_t s) {
    uint64_t base = 0;
    FS_TRY(clk.mark(62, s));
    for (uint32_t k = 2; k <= max_length; ++k) {
      if (!f[k].n) continue;
      hipLaunchKernelGGL(k_rt_emit, dim3(blocks_of(f[k].n, kBlock)), dim3(kBlock), 0, s, f[k],
                         d_routes, base);
      base += f[k].n;
    }
    FS_TRY(clk.mark(63, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[kTimes - 2] += clk.elapsed(62, 63);
    return FS_OK;
  }

  void sum_times() {
    double all = 0.0;
    for (int k = 0; k + 1 < kTimes; ++k) all += t_ms[k];
    t_ms[kTimes - 1] = all;
  }
};

// the rules both entry points share
int rt_check(uint64_t n_rows, uint32_t n_script, const void* unit_of, uint32_t n_units,
             uint32_t min_words, uint32_t max_skip, uint32_t min_all, uint32_t max_length,
             const void* units, const void* levels, const void* routes, uint64_t cap,
             uint64_t* n_routes) {
  if (!n_routes || !levels || (n_units && !units) || (cap && !routes) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_all == 0) {
    fs_set_error("min_words and min_all must be at least 1");
    return FS_E_INVALID;
  }
  if (max_length < 2 || max_length > FS_ROUTES_MAX_LENGTH) {
    fs_set_error("max_length %u: 2 to %u", max_length, FS_ROUTES_MAX_LENGTH);
    return FS_E_INVALID;
  }
  if (max_skip > FS_ROUTES_MAX_SKIP && max_skip != FS_NONE) {
    fs_set_error("max_skip %u: 0 to %u, or 0xFFFFFFFF for any distance", max_skip,
                 FS_ROUTES_MAX_SKIP);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("routes", n_rows, n_script));
  *n_routes = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_routes(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                         uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                         uint32_t min_words, uint32_t max_gap, uint32_t max_skip,
                         uint32_t min_all, uint32_t max_length, fs_route_unit* units,
                         fs_route_level* levels, fs_route* routes, uint64_t cap,
                         uint64_t* n_routes) {
  FS_TRY(rt_check(n_rows, n_script, unit_of, n_units, min_words, max_skip, min_all, max_length,
                  units, levels, routes, cap, n_routes));
  RtJob job;
  if (!n_rows || !n_units) {
    job.max_length = max_length;
    job.blank_levels();
    for (double& t : t_ms) t = 0.0;
    const fs_route_unit none{0u, 0u, 0u, 0u};
    for (uint32_t u = 0; u < n_units; ++u) units[u] = none;
    for (uint32_t k = 0; k < max_length; ++k) levels[k] = job.levels[k];
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
  DBuf<fs_route_unit> d_units;
  DBuf<fs_route> d_routes;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n_script, nullptr));
  FS_TRY(d_units.reserve(n_units));
  FS_TRY(job.mine(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap,
                  max_skip, min_all, max_length, d_units.p, nullptr));
  FS_TRY(copy_out(units, d_units, n_units));
  for (uint32_t k = 0; k < max_length; ++k) levels[k] = job.levels[k];
  *n_routes = job.n_routes;
  job.sum_times();
  if (job.n_routes > cap) return FS_E_CAPACITY;
  if (job.n_routes) {
    FS_TRY(d_routes.reserve(job.n_routes));
    FS_TRY(job.write(d_routes.p, nullptr));
    FS_TRY(copy_out(routes, d_routes, job.n_routes));
    job.sum_times();
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_routes_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                              uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                              uint32_t min_words, uint32_t max_gap, uint32_t max_skip,
                              uint32_t min_all, uint32_t max_length, fs_route_unit* d_units,
                              fs_route_level* d_levels, fs_route* d_routes, uint64_t cap,
                              uint64_t* n_routes) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: routes take up to %u", (u64)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(rt_check(n_rows, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, max_skip,
                  min_all, max_length, d_units, d_levels, d_routes, cap, n_routes));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 15) || ((uintptr_t)d_levels & 7) || ((uintptr_t)d_routes & 15)) {
    fs_set_error("d_rows, d_units and d_routes must be 16-byte aligned device pointers, "
                 "d_levels 8-byte and d_unit_of 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  RtJob job;
  FS_TRY(job.mine(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                  min_words, max_gap, max_skip, min_all, max_length, d_units, ix->stream));
  FS_HIP(hipMemcpyAsync(d_levels, job.levels, max_length * sizeof(fs_route_level),
                        hipMemcpyHostToDevice, ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  *n_routes = job.n_routes;
  job.sum_times();
  if (job.n_routes > cap) return FS_E_CAPACITY;
  if (job.n_routes) FS_TRY(job.write(d_routes, ix->stream));
  job.sum_times();
  return FS_OK;
}

extern "C" int fs_routes_times(double* ms) {
  return times_out(ms, t_ms, kTimes);
}
