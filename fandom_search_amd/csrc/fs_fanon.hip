// fs_fanon.hip -- `ao3.py fanon`: the phrases fan works share with each other and the script
// lacks (fs_fanon, fs_fanon_dev in include/fandom_search.h).  The one unit that reads the corpus
// itself: every position of every work is hashed with its K - 1 followers and entered into one
// open-addressing table, the scripts' grams in front of them; what a gram's slot then knows
// (first position, occurrences, works, canon) flags every position, runs of shared positions
// are the passages, and equal passages are grouped into phrases as fs_readings groups its
// readings.
//
// Nothing is sorted: every order is an order of positions, so firsts are flagged, counted per
// workgroup, scanned and placed.  Equal hashes are settled by comparing the ids, so the result
// does not depend on the hash (FS_FANON_HASH_BITS cuts it down to prove that).  A gram's first
// position and a phrase's first passage are atomicMins, counts are atomicAdds, distinct works
// come from the set primitive of fs_probe.h over (slot, work): no schedule changes a result.
// Separate launches; no workgroup waits on another:
//   k_fn_canon        one lane per script position: its gram entered, the slot marked canon
//   k_fn_insert       a workgroup per FS_FANON_TILE positions: the ids and their halo in LDS,
//                     one lane per position hashes, enters and counts; the ids are checked here
//   k_fn_flag         one lane per position: shared / canon / common from its slot, and the two
//                     cover masks (a bit per position) by ballot
//   k_fn_marks        run starts, run ends and first positions of shared grams: counted per
//                     workgroup, then (after k_fn_scan) placed in position order
//   k_fn_phrase       one wave per passage: least and most, the hash of its ids, the phrase
//                     table (k_rd_insert's shape), the per-work passage count and longest
//   k_fn_heads        phrases counted and placed in order of their first passage
//   k_fn_passages     the passage records
//   k_fn_works        one wave per work: its counts and the two token unions, each a windowed
//                     OR over a cover mask
#include "fs_internal.h"
#include "fs_probe.h"
#include "fs_prims.h"

#include <vector>

namespace {

constexpr uint32_t kBlock = FS_FANON_TILE;
constexpr uint32_t kHalo = FS_FANON_MAX_LENGTH;     // K - 1 < 32 ids behind a tile
constexpr uint64_t kMul = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kShared = 1, kCanon = 2, kCommon = 4;

static_assert(sizeof(fs_fanon_work) == 40 && sizeof(fs_fanon_gram) == 16 &&
              sizeof(fs_fanon_passage) == 24 && sizeof(fs_fanon_phrase) == 32, "fs_fanon");
static_assert(FS_FANON_NO_ID == FS_NONE, "fs_fanon");

struct FnArgs {
  const uint32_t* tok;           // [n_tok]
  const uint64_t* work_off;      // [n_works + 1]
  const uint32_t* canon;         // [n_canon]
  const uint64_t* canon_off;     // [n_scripts + 1]
  uint32_t n_tok, n_works, n_ids, n_canon, n_scripts, k, min_works, max_share;
  uint32_t n_pass;
  uint64_t mask, wmask;          // slots - 1 of the gram table and of the (gram, work) set
  uint64_t pmask;                // slots - 1 of the phrase table and of the (phrase, work) set
  uint64_t hash_mask;            // FS_FANON_HASH_BITS: the bits of a hash kept
  unsigned long long* g_tab;     // tag << 32 | position that claimed the slot (a script's: n_tok + q)
  unsigned long long* gw_tab;    // gram slot << 32 | work
  uint32_t* g_first;             // [slots] smallest fan position of the gram
  uint32_t* g_occ;               //         its positions
  uint32_t* g_nw;                //         its works
  uint8_t* g_canon;              //         1: a script holds it
  uint32_t* slot_of;             // [n_tok] the slot of the position's gram, FS_NONE without one
  uint8_t* flag;                 // [n_tok] kShared | kCanon | kCommon
  unsigned long long* m_shared;  // [workgroups * kBlock / 64] bit i & 63 of word i >> 6: position i shared
  unsigned long long* m_canon;   //                           the same for canon
  uint32_t* cnt_g;               // [workgroups] first positions of shared grams, then their scan
  uint32_t* cnt_s;               //              run starts
  uint32_t* cnt_e;               //              run ends
  uint32_t* p_start;             // [n_pass] first and last position of the run
  uint32_t* p_end;
  uint32_t* p_slot;              // [n_pass] slot of its phrase
  uint2* p_lm;                   // [n_pass] least, most
  unsigned long long* p_tab;     // tag << 32 | passage that claimed the slot
  unsigned long long* pw_tab;    // phrase slot << 32 | work
  uint32_t* ph_first;            // [pslots] smallest passage of the phrase
  uint32_t* ph_np;               //          its passages
  uint32_t* ph_nw;               //          its works
  uint32_t* ph_id;               //          its place in the output
  uint32_t* cnt_p;               // [workgroups of passages] phrase heads, then their scan
  uint32_t* w_np;                // [n_works] passages of the work
  unsigned long long* w_long;    // [n_works] n_tokens << 32 | ~start of its longest passage
  uint32_t* status;              // [0] invalid input, [1] total of the last scan, [2] distinct grams
  fs_fanon_work* works;
  fs_fanon_gram* grams;
  fs_fanon_passage* passages;
  fs_fanon_phrase* phrases;
};

// the w < n with off[w] <= i < off[w + 1], for i < off[n]: empty ranges are passed over
__device__ inline uint32_t range_of(const uint64_t* __restrict__ off, uint32_t n, uint64_t i) {
  uint32_t lo = 0, hi = n;                 // off[lo] <= i < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// the id at position u of the fan tokens with the scripts' words behind them
__device__ inline uint32_t id_at(const FnArgs& a, uint32_t u) {
  return u < a.n_tok ? a.tok[u] : a.canon[u - a.n_tok];
}

// The slot of the gram at position u, whose ids are id(0) .. id(k - 1); *inserted when this
// call claimed it.
template <class Id>
__device__ inline uint32_t gram_slot(const FnArgs& a, uint32_t u, Id id, bool* inserted) {
  uint64_t h = a.k;
  for (uint32_t j = 0; j < a.k; ++j) h = h * kMul + id(j) + 1;
  h = fs_mix64(fs_mix64(h) & a.hash_mask);         // the kept bits decide slot and tag
  const uint32_t tag = (uint32_t)(h >> 32);
  const unsigned long long mine = (unsigned long long)tag << 32 | u;
  return (uint32_t)fs_probe_insert(
      a.g_tab, a.mask, h, mine,
      [&a, &id, tag, u](unsigned long long cur) {
        if ((uint32_t)(cur >> 32) != tag) return false;
        const uint32_t o = (uint32_t)cur;
        if (o == u) return true;
        for (uint32_t j = 0; j < a.k; ++j)
          if (id(j) != id_at(a, o + j)) return false;
        return true;
      },
      inserted);
}

__global__ __launch_bounds__(kBlock) void k_fn_canon(FnArgs a) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  const bool live = q < a.n_canon;
  const uint32_t mine = live ? a.canon[q] : 0;
  const bool bad = live && mine != FS_NONE && mine >= a.n_ids;
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 1u);
  if (!live) return;
  const uint32_t s = range_of(a.canon_off, a.n_scripts, q);
  if ((uint64_t)q + a.k > a.canon_off[s + 1]) return;
  for (uint32_t j = 0; j < a.k; ++j)
    if (a.canon[q + j] == FS_NONE) return;         // no fan gram equals it
  const uint32_t* ids = a.canon + q;
  bool inserted;
  const uint32_t slot = gram_slot(a, a.n_tok + q, [ids](uint32_t j) { return ids[j]; }, &inserted);
  a.g_canon[slot] = 1;
}

__global__ __launch_bounds__(kBlock) void k_fn_insert(FnArgs a) {
  __shared__ uint32_t s_ids[kBlock + kHalo];
  const uint32_t t = threadIdx.x;
  const uint64_t base = (uint64_t)blockIdx.x * kBlock;
  const uint64_t i = base + t;
  const bool live = i < a.n_tok;
  s_ids[t] = live ? a.tok[i] : 0;
  if (t < kHalo) {
    const uint64_t j = base + kBlock + t;
    s_ids[kBlock + t] = j < a.n_tok ? a.tok[j] : 0;
  }
  __syncthreads();
  const bool bad = live && s_ids[t] >= a.n_ids;
  if (__ballot(bad) && (t & 63) == 0) atomicOr(&a.status[0], 1u);
  if (!live) return;
  const uint32_t w = range_of(a.work_off, a.n_works, i);
  uint32_t slot = FS_NONE;
  if (i + a.k <= a.work_off[w + 1]) {              // the gram ends inside the work (and the tile's halo)
    const uint32_t* ids = s_ids + t;
    bool inserted;
    slot = gram_slot(a, (uint32_t)i, [ids](uint32_t j) { return ids[j]; }, &inserted);
    atomicAdd(&a.g_occ[slot], 1u);
    // a value read here is never below the slot's final one: a position at or above it need not try
    if ((uint32_t)i < ld_agent(&a.g_first[slot])) atomicMin(&a.g_first[slot], (uint32_t)i);
    const unsigned long long key = (unsigned long long)slot << 32 | w;
    fs_probe_insert(a.gw_tab, a.wmask, fs_mix64(key), key,
                    [key](unsigned long long cur) { return cur == key; }, &inserted);
    if (inserted) atomicAdd(&a.g_nw[slot], 1u);
  }
  a.slot_of[i] = slot;
}

__global__ __launch_bounds__(kBlock) void k_fn_flag(FnArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t f = 0;
  if (i < a.n_tok) {
    const uint32_t slot = a.slot_of[i];
    if (slot != FS_NONE) {
      const uint32_t nw = a.g_nw[slot];
      const bool canon = a.g_canon[slot] != 0;
      const bool common = (uint64_t)nw * 100u > (uint64_t)a.max_share * a.n_works;
      f = (canon ? kCanon : 0u) | (common ? kCommon : 0u);
      if (!canon && !common && nw >= a.min_works) f |= kShared;
    }
    a.flag[i] = (uint8_t)f;
  }
  const uint64_t sh = __ballot((f & kShared) != 0), ca = __ballot((f & kCanon) != 0);
  if ((threadIdx.x & 63) == 0) {                   // every word of the masks is written: i >> 6 is this wave
    a.m_shared[i >> 6] = sh;
    a.m_canon[i >> 6] = ca;
  }
}

__global__ __launch_bounds__(kScanBlock) void k_fn_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t nb, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, nb, out, total);
}

// kMode 0: this workgroup's run starts, run ends and first positions of shared grams into cnt_*
// (and the distinct grams into status[2]); 1: the runs placed, cnt_s and cnt_e holding the
// scans; 2: the gram records placed, cnt_g holding the scan
template <int kMode>
__global__ __launch_bounds__(kBlock) void k_fn_marks(FnArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < a.n_tok;
  const uint32_t f = live ? a.flag[i] : 0u;
  const bool shared = (f & kShared) != 0;
  uint32_t rank, total;
  if (kMode != 2) {
    // a work's last K - 1 positions hold no gram: a run never crosses into the next work
    const bool prev = live && i > 0 && (a.flag[i - 1] & kShared);
    const bool next = live && i + 1 < a.n_tok && (a.flag[i + 1] & kShared);
    const bool start = shared && !prev, end = shared && !next;
    block_rank<kBlock>(start, s_w, &rank, &total);
    if (kMode == 0 && threadIdx.x == 0) a.cnt_s[blockIdx.x] = total;
    if (kMode == 1 && start) a.p_start[a.cnt_s[blockIdx.x] + rank] = (uint32_t)i;
    block_rank<kBlock>(end, s_w, &rank, &total);
    if (kMode == 0 && threadIdx.x == 0) a.cnt_e[blockIdx.x] = total;
    if (kMode == 1 && end) a.p_end[a.cnt_e[blockIdx.x] + rank] = (uint32_t)i;
  }
  if (kMode != 1) {
    const uint32_t slot = live ? a.slot_of[i] : FS_NONE;
    const bool own = slot != FS_NONE && a.g_first[slot] == (uint32_t)i;
    block_rank<kBlock>(own && shared, s_w, &rank, &total);
    if (kMode == 0) {
      if (threadIdx.x == 0) a.cnt_g[blockIdx.x] = total;
      const uint64_t b = __ballot(own);
      if (b && (threadIdx.x & 63) == 0) atomicAdd(&a.status[2], (uint32_t)__popcll(b));
    } else if (own && shared) {
      const uint32_t w = range_of(a.work_off, a.n_works, i);
      a.grams[a.cnt_g[blockIdx.x] + rank] =
          fs_fanon_gram{w, (uint32_t)(i - a.work_off[w]), a.g_nw[slot], a.g_occ[slot]};
    }
  }
}

// the id sequences of passages x and y (wave-uniform) are equal; the whole wave compares
__device__ inline bool same_phrase(const FnArgs& a, uint32_t x, uint32_t nx, uint32_t y,
                                   uint32_t ny, uint32_t lane) {
  if (nx != ny) return false;
  for (uint32_t c = 0; c < nx; c += 64) {
    const uint32_t i = c + lane;
    const bool differ = i < nx && a.tok[x + i] != a.tok[y + i];
    if (__ballot(differ)) return false;
  }
  return true;
}

__global__ __launch_bounds__(kBlock) void k_fn_phrase(FnArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (p >= a.n_pass) return;
  const uint32_t b = a.p_start[p], e = a.p_end[p];
  const uint32_t n = e - b + a.k;
  const uint32_t w = range_of(a.work_off, a.n_works, b);
  uint32_t least = FS_NONE, most = 0;
  for (uint64_t i = (uint64_t)b + lane; i <= e; i += 64) {
    const uint32_t nw = a.g_nw[a.slot_of[i]];
    least = nw < least ? nw : least;
    most = nw > most ? nw : most;
  }
  least = ~wave_max(~least);
  most = wave_max(most);
  // a sum over the tokens of a mix of (place, id): the order of the lanes' parts does not matter
  uint64_t acc = 0;
  for (uint32_t i = lane; i < n; i += 64)
    acc += fs_mix64(a.tok[b + i] + (uint64_t)(i + 1) * kMul);
  acc = wave_sum(acc);
  uint64_t h = acc ^ fs_mix64(n);
  h = fs_mix64(fs_mix64(h) & a.hash_mask);
  const uint32_t tag = (uint32_t)(h >> 32);
  const unsigned long long mine = (unsigned long long)tag << 32 | p;

  // the slot of this phrase: lane 0 reads or claims, the wave compares (fs_probe.h's loop)
  uint64_t pos = h & a.pmask;
  for (;; pos = (pos + 1) & a.pmask) {
    unsigned long long cur = 0;
    if (lane == 0) {
      cur = __hip_atomic_load(&a.p_tab[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kProbeEmpty) {
        cur = atomicCAS(&a.p_tab[pos], kProbeEmpty, mine);
        if (cur == kProbeEmpty) cur = mine;
      }
    }
    cur = wave_first(cur);
    if (cur == mine) break;
    if ((uint32_t)(cur >> 32) == tag) {
      const uint32_t o = (uint32_t)cur;
      const uint32_t ob = a.p_start[o];
      if (same_phrase(a, b, n, ob, a.p_end[o] - ob + a.k, lane)) break;
    }
  }
  if (lane == 0) {
    const uint32_t slot = (uint32_t)pos;
    a.p_slot[p] = slot;
    a.p_lm[p] = make_uint2(least, most);
    if (p < ld_agent(&a.ph_first[slot])) atomicMin(&a.ph_first[slot], p);
    atomicAdd(&a.ph_np[slot], 1u);
    const unsigned long long key = (unsigned long long)slot << 32 | w;
    bool inserted;
    fs_probe_insert(a.pw_tab, a.pmask, fs_mix64(key), key,
                    [key](unsigned long long cur) { return cur == key; }, &inserted);
    if (inserted) atomicAdd(&a.ph_nw[slot], 1u);
    atomicAdd(&a.w_np[w], 1u);
    // the longest, then the earliest: the largest n_tokens << 32 | ~start
    atomicMax(&a.w_long[w], (unsigned long long)n << 32 | (uint32_t)~(uint32_t)(b - a.work_off[w]));
  }
}

// kPlace false: the phrase heads (passages that are their phrase's first) of this workgroup's
// passages into cnt_p; true: the phrase records to their places, cnt_p holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_fn_heads(FnArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t slot = p < a.n_pass ? a.p_slot[p] : 0;
  const bool head = p < a.n_pass && a.ph_first[slot] == p;
  uint32_t rank, total;
  block_rank<kBlock>(head, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.cnt_p[blockIdx.x] = total;
  } else if (head) {
    const uint32_t r = a.cnt_p[blockIdx.x] + rank;
    const uint32_t b = a.p_start[p];
    const uint32_t w = range_of(a.work_off, a.n_works, b);
    const uint2 lm = a.p_lm[p];
    a.ph_id[slot] = r;
    a.phrases[r] = fs_fanon_phrase{w, (uint32_t)(b - a.work_off[w]), a.p_end[p] - b + a.k,
                                   a.ph_np[slot], a.ph_nw[slot], lm.x, lm.y, 0u};
  }
}

__global__ __launch_bounds__(kBlock) void k_fn_passages(FnArgs a) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= a.n_pass) return;
  const uint32_t b = a.p_start[p];
  const uint32_t w = range_of(a.work_off, a.n_works, b);
  const uint2 lm = a.p_lm[p];
  a.passages[p] = fs_fanon_passage{w, (uint32_t)(b - a.work_off[w]), a.p_end[p] - b + a.k,
                                   a.ph_id[a.p_slot[p]], lm.x, lm.y};
}

// token t lies inside the gram of a flagged position: a bit among t - K + 1 .. t of the mask.
// (Positions in front of the work's start that near hold no gram, so the window needs no clip.)
__device__ inline bool covered(const unsigned long long* __restrict__ m, uint64_t t, uint32_t k) {
  const uint32_t bit = (uint32_t)(t & 63);
  const unsigned long long cur = m[t >> 6];
  const unsigned long long prev = (bit < 63 && (t >> 6)) ? m[(t >> 6) - 1] : 0ull;
  // bit 63 - j of y: position t - j
  const unsigned long long y = cur << (63 - bit) | (bit < 63 ? prev >> (bit + 1) : 0ull);
  return (y >> (64 - k)) != 0;
}

__global__ __launch_bounds__(kBlock) void k_fn_works(FnArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (w >= a.n_works) return;
  const uint64_t b = a.work_off[w], e = a.work_off[w + 1];
  uint32_t n_sh = 0, n_ca = 0, n_co = 0, t_sh = 0, t_ca = 0;
  for (uint64_t t = b + lane; t < e; t += 64) {
    const uint32_t f = a.flag[t];
    n_sh += (f & kShared) ? 1u : 0u;
    n_ca += (f & kCanon) ? 1u : 0u;
    n_co += (f & kCommon) ? 1u : 0u;
    t_sh += covered(a.m_shared, t, a.k) ? 1u : 0u;
    t_ca += covered(a.m_canon, t, a.k) ? 1u : 0u;
  }
  n_sh = wave_sum(n_sh);
  n_ca = wave_sum(n_ca);
  n_co = wave_sum(n_co);
  t_sh = wave_sum(t_sh);
  t_ca = wave_sum(t_ca);
  if (lane == 0) {
    const uint32_t len = (uint32_t)(e - b);
    const unsigned long long lg = a.w_long[w];
    fs_fanon_work r;
    r.n_tokens = len;
    r.n_positions = len >= a.k ? len - a.k + 1 : 0u;
    r.shared_positions = n_sh;
    r.canon_positions = n_ca;
    r.common_positions = n_co;
    r.n_passages = a.w_np[w];
    r.shared_tokens = t_sh;
    r.canon_tokens = t_ca;
    r.longest_start = lg ? ~(uint32_t)lg : 0u;
    r.longest_tokens = (uint32_t)(lg >> 32);
    a.works[w] = r;
  }
}

uint64_t fanon_hash_mask() {
  const char* e = getenv("FS_FANON_HASH_BITS");    // diagnostic: k bits of a hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1;
}

uint64_t fanon_max_bytes() {
  const char* e = getenv("FS_FANON_MAX_BYTES");
  if (!e || !*e) return FS_FANON_MAX_BYTES;
  return strtoull(e, nullptr, 10);
}

// offsets ascend from 0; *positions = the places of n ranges where k items fit
bool offsets_ok(const uint64_t* off, uint32_t n, uint32_t k, uint64_t* positions) {
  *positions = 0;
  if (off[0] != 0) return false;
  for (uint32_t w = 0; w < n; ++w) {
    if (off[w + 1] < off[w]) return false;
    const uint64_t len = off[w + 1] - off[w];
    if (len >= k) *positions += len - k + 1;
  }
  return true;
}

int too_large(const char* what, uint64_t need, uint64_t most) {
  fs_set_error("%s need %llu bytes, more than FS_FANON_MAX_BYTES = %llu: lower -n", what,
               (unsigned long long)need, (unsigned long long)most);
  return FS_E_UNSUPPORTED;
}

// insert, flag, phrases, place, works, copy out, total of the last call
thread_local double t_ms[7];

struct FnOut {
  fs_fanon_work* works;
  fs_fanon_gram* grams;
  fs_fanon_passage* passages;
  fs_fanon_phrase* phrases;
  uint64_t cap_grams, cap_passages, cap_phrases;
  uint64_t *n_grams, *n_passages, *n_phrases, *n_positions, *n_distinct;
};

// The passes over device-resident ids and offsets; h_off and h_coff are the offsets on the host,
// checked.  to_host: `out` names host buffers, filled through buffers of this call; else device
// buffers, written in place.
int fanon_job(const uint32_t* d_tok, const uint64_t* d_off, const uint64_t* h_off,
              uint32_t n_works, uint32_t n_ids, const uint32_t* d_canon, const uint64_t* d_coff,
              const uint64_t* h_coff, uint32_t n_scripts, uint32_t k, uint32_t min_works,
              uint32_t max_share, uint64_t positions, uint64_t canon_positions, bool to_host,
              const FnOut& out) {
  FnArgs a{};
  a.tok = d_tok;
  a.work_off = d_off;
  a.canon = d_canon;
  a.canon_off = d_coff;
  a.n_tok = (uint32_t)h_off[n_works];
  a.n_works = n_works;
  a.n_ids = n_ids;
  a.n_scripts = n_scripts;
  a.n_canon = n_scripts ? (uint32_t)h_coff[n_scripts] : 0u;
  a.k = k;
  a.min_works = min_works;
  a.max_share = max_share;
  a.hash_mask = fanon_hash_mask();
  const uint64_t most = fanon_max_bytes();
  const uint32_t blocks = blocks_of(a.n_tok, kBlock);
  const uint64_t slots = fs_probe_slots(positions + canon_positions);
  const uint64_t wslots = fs_probe_slots(positions);
  const uint64_t mwords = (uint64_t)blocks * (kBlock / 64);
  const uint64_t need = (uint64_t)a.n_tok * 5 + mwords * 16 + slots * FS_FANON_SLOT_BYTES +
                        wslots * 8 + (uint64_t)blocks * 12 + (uint64_t)n_works * 12;
  if (need > most || slots > (1ull << 31)) return too_large("the gram tables", need, most);

  DBuf<uint32_t> d_status, d_slot_of, d_gz, d_first, d_cnt, d_wnp;
  DBuf<uint8_t> d_flag, d_gcanon;
  DBuf<unsigned long long> d_keys, d_masks, d_wlong;
  FS_TRY(d_status.reserve(4));
  FS_TRY(d_slot_of.reserve(a.n_tok));
  FS_TRY(d_flag.reserve(a.n_tok));
  FS_TRY(d_keys.reserve(slots + wslots));
  FS_TRY(d_first.reserve(slots));
  FS_TRY(d_gz.reserve(2 * slots));
  FS_TRY(d_gcanon.reserve(slots));
  FS_TRY(d_masks.reserve(2 * mwords));
  FS_TRY(d_cnt.reserve(3 * (size_t)blocks));
  FS_TRY(d_wnp.reserve(n_works));
  FS_TRY(d_wlong.reserve(n_works));
  FS_HIP(hipMemsetAsync(d_status.p, 0, 4 * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_keys.p, 0xFF, (slots + wslots) * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_first.p, 0xFF, slots * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_gz.p, 0, 2 * slots * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_gcanon.p, 0, slots, nullptr));
  FS_HIP(hipMemsetAsync(d_wnp.p, 0, (size_t)n_works * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_wlong.p, 0, (size_t)n_works * sizeof(unsigned long long), nullptr));
  a.status = d_status.p;
  a.slot_of = d_slot_of.p;
  a.flag = d_flag.p;
  a.mask = slots - 1;
  a.wmask = wslots - 1;
  a.g_tab = d_keys.p;
  a.gw_tab = d_keys.p + slots;
  a.g_first = d_first.p;
  a.g_occ = d_gz.p;
  a.g_nw = d_gz.p + slots;
  a.g_canon = d_gcanon.p;
  a.m_shared = d_masks.p;
  a.m_canon = d_masks.p + mwords;
  a.cnt_g = d_cnt.p;
  a.cnt_s = d_cnt.p + blocks;
  a.cnt_e = d_cnt.p + 2 * (size_t)blocks;
  a.w_np = d_wnp.p;
  a.w_long = d_wlong.p;

  Clock<7> clk;
  FS_TRY(clk.mark(0, nullptr));
  if (a.n_canon)
    hipLaunchKernelGGL(k_fn_canon, dim3(blocks_of(a.n_canon, kBlock)), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_fn_insert, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(1, nullptr));
  uint32_t st[4];
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) {
    fs_set_error("a tok[i] >= n_ids, or a canon id that is neither below n_ids nor FS_FANON_NO_ID");
    return FS_E_INVALID;
  }

  // flags, cover masks, and the three counts in position order
  hipLaunchKernelGGL(k_fn_flag, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_fn_marks<0>, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  uint32_t n_grams = 0, n_ends = 0;
  uint32_t* const cnts[3] = {a.cnt_g, a.cnt_e, a.cnt_s};
  uint32_t* const tots[3] = {&n_grams, &n_ends, &a.n_pass};
  for (int c = 0; c < 3; ++c) {
    hipLaunchKernelGGL(k_fn_scan, dim3(1), dim3(kScanBlock), 0, nullptr, cnts[c], cnts[c], blocks,
                       a.status + 1);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
    *tots[c] = st[1];
  }
  *out.n_grams = n_grams;
  *out.n_passages = a.n_pass;
  if (out.n_distinct) *out.n_distinct = st[2];
  if (n_ends != a.n_pass) {
    fs_set_error("%u run starts and %u run ends", a.n_pass, n_ends);
    return FS_E_DEVICE;
  }

  // the runs, and their phrases
  const uint64_t pslots = fs_probe_slots(a.n_pass);
  const uint32_t pass_blocks = blocks_of(a.n_pass, kBlock);
  const uint64_t pneed = need + (uint64_t)a.n_pass * 20 + pslots * FS_FANON_PHRASE_SLOT_BYTES +
                         (uint64_t)pass_blocks * 4;
  if (pneed > most) return too_large("the gram and phrase tables", pneed, most);
  DBuf<uint32_t> d_pass, d_pz, d_pfirst, d_cntp;
  DBuf<uint2> d_plm;
  DBuf<unsigned long long> d_pkeys;
  FS_TRY(d_pass.reserve(3 * (size_t)a.n_pass));
  FS_TRY(d_plm.reserve(a.n_pass));
  FS_TRY(d_pkeys.reserve(2 * pslots));
  FS_TRY(d_pfirst.reserve(pslots));
  FS_TRY(d_pz.reserve(3 * pslots));
  FS_TRY(d_cntp.reserve(pass_blocks));
  FS_HIP(hipMemsetAsync(d_pkeys.p, 0xFF, 2 * pslots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_pfirst.p, 0xFF, pslots * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_pz.p, 0, 3 * pslots * sizeof(uint32_t), nullptr));
  a.p_start = d_pass.p;
  a.p_end = d_pass.p + a.n_pass;
  a.p_slot = d_pass.p + 2 * (size_t)a.n_pass;
  a.p_lm = d_plm.p;
  a.pmask = pslots - 1;
  a.p_tab = d_pkeys.p;
  a.pw_tab = d_pkeys.p + pslots;
  a.ph_first = d_pfirst.p;
  a.ph_np = d_pz.p;
  a.ph_nw = d_pz.p + pslots;
  a.ph_id = d_pz.p + 2 * pslots;
  a.cnt_p = d_cntp.p;
  uint32_t n_phrases = 0;
  if (a.n_pass) {
    hipLaunchKernelGGL(k_fn_marks<1>, dim3(blocks), dim3(kBlock), 0, nullptr, a);
    FS_HIP(hipGetLastError());
    FS_TRY(clk.mark(2, nullptr));
    hipLaunchKernelGGL(k_fn_phrase, dim3(blocks_of(a.n_pass, kBlock / 64)), dim3(kBlock), 0,
                       nullptr, a);
    hipLaunchKernelGGL(k_fn_heads<false>, dim3(pass_blocks), dim3(kBlock), 0, nullptr, a);
    hipLaunchKernelGGL(k_fn_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.cnt_p, a.cnt_p,
                       pass_blocks, a.status + 1);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
    n_phrases = st[1];
  } else {
    FS_TRY(clk.mark(2, nullptr));
  }
  *out.n_phrases = n_phrases;
  FS_TRY(clk.mark(3, nullptr));

  // the records
  DBuf<fs_fanon_work> o_works;
  DBuf<fs_fanon_gram> o_grams;
  DBuf<fs_fanon_passage> o_passages;
  DBuf<fs_fanon_phrase> o_phrases;
  const bool fits = n_grams <= out.cap_grams && a.n_pass <= out.cap_passages &&
                    n_phrases <= out.cap_phrases;
  a.works = out.works;
  a.grams = out.grams;
  a.passages = out.passages;
  a.phrases = out.phrases;
  if (to_host) {
    FS_TRY(o_works.reserve(n_works));
    a.works = o_works.p;
    if (fits) {
      FS_TRY(o_grams.reserve(n_grams));
      FS_TRY(o_passages.reserve(a.n_pass));
      FS_TRY(o_phrases.reserve(n_phrases));
      a.grams = o_grams.p;
      a.passages = o_passages.p;
      a.phrases = o_phrases.p;
    }
  }
  if (fits && n_grams) hipLaunchKernelGGL(k_fn_marks<2>, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  if (fits && a.n_pass) {
    hipLaunchKernelGGL(k_fn_heads<true>, dim3(pass_blocks), dim3(kBlock), 0, nullptr, a);
    hipLaunchKernelGGL(k_fn_passages, dim3(pass_blocks), dim3(kBlock), 0, nullptr, a);
  }
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, nullptr));
  hipLaunchKernelGGL(k_fn_works, dim3(blocks_of(n_works, kBlock / 64)), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(5, nullptr));
  if (to_host) {
    FS_HIP(hipMemcpyAsync(out.works, o_works.p, (size_t)n_works * sizeof(fs_fanon_work),
                          hipMemcpyDeviceToHost, nullptr));
    if (fits) {
      FS_HIP(hipMemcpyAsync(out.grams, o_grams.p, (size_t)n_grams * sizeof(fs_fanon_gram),
                            hipMemcpyDeviceToHost, nullptr));
      FS_HIP(hipMemcpyAsync(out.passages, o_passages.p,
                            (size_t)a.n_pass * sizeof(fs_fanon_passage), hipMemcpyDeviceToHost,
                            nullptr));
      FS_HIP(hipMemcpyAsync(out.phrases, o_phrases.p, (size_t)n_phrases * sizeof(fs_fanon_phrase),
                            hipMemcpyDeviceToHost, nullptr));
    }
  }
  FS_TRY(clk.mark(6, nullptr));
  FS_HIP(hipDeviceSynchronize());
  for (int c = 0; c < 6; ++c) t_ms[c] = clk.elapsed(c, c + 1);
  t_ms[6] = clk.elapsed(0, 6);
  if (!fits) {
    fs_set_error("%u grams, %u passages and %u phrases need room", n_grams, a.n_pass, n_phrases);
    return FS_E_CAPACITY;
  }
  return FS_OK;
}

// what both entry points refuse before anything is read
int fanon_params(uint32_t n_works, uint32_t n_scripts, uint32_t k, uint32_t min_works,
                 uint32_t max_share, const FnOut& out, const void* work_off, const void* canon,
                 const void* canon_off) {
  if (!out.n_grams || !out.n_passages || !out.n_phrases || !work_off || (n_works && !out.works) ||
      (out.cap_grams && !out.grams) || (out.cap_passages && !out.passages) ||
      (out.cap_phrases && !out.phrases) || (n_scripts && (!canon_off || !canon))) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (k < FS_FANON_MIN_LENGTH || k > FS_FANON_MAX_LENGTH) {
    fs_set_error("k %u: a gram has %u to %u tokens", k, FS_FANON_MIN_LENGTH, FS_FANON_MAX_LENGTH);
    return FS_E_INVALID;
  }
  if (min_works == 0) {
    fs_set_error("min_works must be at least 1");
    return FS_E_INVALID;
  }
  if (max_share < 1 || max_share > 100) {
    fs_set_error("max_share %u: from 1 to 100", max_share);
    return FS_E_INVALID;
  }
  *out.n_grams = *out.n_passages = *out.n_phrases = 0;
  if (out.n_positions) *out.n_positions = 0;
  if (out.n_distinct) *out.n_distinct = 0;
  return FS_OK;
}

// the offsets of both sides: ascending from 0, fewer than 2^32 ids together
int fanon_offsets(const uint64_t* work_off, uint32_t n_works, const uint64_t* canon_off,
                  uint32_t n_scripts, uint32_t k, uint64_t* positions, uint64_t* canon_positions) {
  *canon_positions = 0;
  if (!offsets_ok(work_off, n_works, k, positions) ||
      (n_scripts && !offsets_ok(canon_off, n_scripts, k, canon_positions))) {
    fs_set_error("offsets that do not ascend from 0");
    return FS_E_INVALID;
  }
  const uint64_t n_canon = n_scripts ? canon_off[n_scripts] : 0;
  if (work_off[n_works] >= (1ull << 32) || n_canon >= (1ull << 32) ||
      work_off[n_works] + n_canon >= (1ull << 32)) {
    fs_set_error("%llu tokens and %llu script words: fanon takes fewer than 2^32 together",
                 (unsigned long long)work_off[n_works], (unsigned long long)n_canon);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

// the work records of a corpus without a position
void fanon_empty(const uint64_t* work_off, uint32_t n_works, fs_fanon_work* works) {
  for (uint32_t w = 0; w < n_works; ++w) {
    works[w] = fs_fanon_work{};
    works[w].n_tokens = (uint32_t)(work_off[w + 1] - work_off[w]);
  }
}

}  // namespace

extern "C" int fs_fanon(int device, const uint32_t* tok, const uint64_t* work_off,
                        uint32_t n_works, uint32_t n_ids, const uint32_t* canon,
                        const uint64_t* canon_off, uint32_t n_scripts, uint32_t k,
                        uint32_t min_works, uint32_t max_share, fs_fanon_work* works,
                        fs_fanon_gram* grams, uint64_t cap_grams, fs_fanon_passage* passages,
                        uint64_t cap_passages, fs_fanon_phrase* phrases, uint64_t cap_phrases,
                        uint64_t* n_grams, uint64_t* n_passages, uint64_t* n_phrases,
                        uint64_t* n_positions, uint64_t* n_distinct) {
  for (double& t : t_ms) t = 0.0;
  const FnOut out{works, grams, passages, phrases, cap_grams, cap_passages, cap_phrases,
                  n_grams, n_passages, n_phrases, n_positions, n_distinct};
  FS_TRY(fanon_params(n_works, n_scripts, k, min_works, max_share, out, work_off, canon, canon_off));
  uint64_t positions, canon_positions;
  FS_TRY(fanon_offsets(work_off, n_works, canon_off, n_scripts, k, &positions, &canon_positions));
  if (work_off[n_works] && !tok) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (n_positions) *n_positions = positions;
  if (!positions) {
    fanon_empty(work_off, n_works, works);
    return FS_OK;
  }
  FS_ENTER(device);
  DBuf<uint32_t> d_tok, d_canon;
  DBuf<uint64_t> d_off, d_coff;
  FS_TRY(d_tok.upload(tok, work_off[n_works], nullptr));
  FS_TRY(d_off.upload(work_off, (size_t)n_works + 1, nullptr));
  if (n_scripts) {
    FS_TRY(d_canon.upload(canon, canon_off[n_scripts], nullptr));
    FS_TRY(d_coff.upload(canon_off, (size_t)n_scripts + 1, nullptr));
  }
  return fanon_job(d_tok.p, d_off.p, work_off, n_works, n_ids, d_canon.p, d_coff.p, canon_off,
                   n_scripts, k, min_works, max_share, positions, canon_positions, true, out);
}

extern "C" int fs_fanon_dev(int device, const uint32_t* d_tok, uint64_t n_tok,
                            const uint64_t* d_work_off, uint32_t n_works, uint32_t n_ids,
                            const uint32_t* d_canon, uint64_t n_canon,
                            const uint64_t* d_canon_off, uint32_t n_scripts, uint32_t k,
                            uint32_t min_works, uint32_t max_share, fs_fanon_work* d_works,
                            fs_fanon_gram* d_grams, uint64_t cap_grams,
                            fs_fanon_passage* d_passages, uint64_t cap_passages,
                            fs_fanon_phrase* d_phrases, uint64_t cap_phrases, uint64_t* n_grams,
                            uint64_t* n_passages, uint64_t* n_phrases, uint64_t* n_positions,
                            uint64_t* n_distinct) {
  for (double& t : t_ms) t = 0.0;
  const FnOut out{d_works, d_grams, d_passages, d_phrases, cap_grams, cap_passages, cap_phrases,
                  n_grams, n_passages, n_phrases, n_positions, n_distinct};
  FS_TRY(fanon_params(n_works, n_scripts, k, min_works, max_share, out, d_work_off, d_canon,
                      d_canon_off));
  FS_ENTER(device);
  // the offsets decide what is read: they are checked on the host
  std::vector<uint64_t> off((size_t)n_works + 1), coff((size_t)n_scripts + 1, 0);
  FS_HIP(hipMemcpy(off.data(), d_work_off, off.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (n_scripts)
    FS_HIP(hipMemcpy(coff.data(), d_canon_off, coff.size() * sizeof(uint64_t),
                     hipMemcpyDeviceToHost));
  uint64_t positions, canon_positions;
  FS_TRY(fanon_offsets(off.data(), n_works, coff.data(), n_scripts, k, &positions,
                       &canon_positions));
  if (off[n_works] != n_tok || coff[n_scripts] != n_canon || (n_tok && !d_tok)) {
    fs_set_error("n_tok or n_canon is not the last offset");
    return FS_E_INVALID;
  }
  if (n_positions) *n_positions = positions;
  if (!positions) {
    std::vector<fs_fanon_work> works(n_works);
    fanon_empty(off.data(), n_works, works.data());
    FS_HIP(hipMemcpy(d_works, works.data(), works.size() * sizeof(fs_fanon_work),
                     hipMemcpyHostToDevice));
    return FS_OK;
  }
  return fanon_job(d_tok, d_work_off, off.data(), n_works, n_ids, d_canon, d_canon_off,
                   coff.data(), n_scripts, k, min_works, max_share, positions, canon_positions,
                   false, out);
}

extern "C" int fs_fanon_times(double* ms) {
  return times_out(ms, t_ms, 7);
}
