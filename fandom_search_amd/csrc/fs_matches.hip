// fs_matches.hip -- the reader of the 12-column match CSV for `ao3.py passages`, `works` and
// `quotes` (fs_matches_open / _read / _labels / _close in include/fandom_search.h): the file's
// bytes in, row index, numeric columns and head flags out.
//
// A '"' toggles quoting, ',' outside quotes ends a field, '\n' outside quotes ends a row (a
// '\r' directly in front belongs to the terminator).  That parity model equals csv.reader only
// under the conditions byte_check and parse_row test; a file that breaks one is "outside" and
// nothing of it is used.  Separate launches, no workgroup waits on another:
//   k_mt_parity    quotes per 16 KiB tile (popcounts of 16-byte loads), their parity
//   k_mt_scan      one workgroup: exclusive scan of the tile parities
//   k_mt_classify  each lane walks its 64 bytes from its starting parity: the structural and
//                  UTF-8 conditions, a bit per byte that starts a non-empty row, rows per tile
//   k_mt_scan      again, over the row counts
//   k_mt_place     row starts, compacted
//   k_mt_rows      one lane per row: field ends, the three integers, the two doubles (fs_dec.h)
//                  and the head flag (FAN_WORK_FILENAME's bytes differ from the row in front);
//                  the bytes come from global memory or, staged by the wave, from LDS
//   k_mt_first / k_mt_differ   the label check of `works` and `quotes`
// fs_matches_intern numbers the distinct spellings of one text column (`ao3.py variants`):
//   k_in_insert    one lane per row: hash of its field, a slot of an open-addressing table of
//                  {tag, row} claimed or found (fs_probe.h; equal tags are compared byte for
//                  byte), atomicMin of the row into the slot's first row
//   k_in_count     rows that are their slot's first row, per 256 rows
//   k_mt_scan      over those counts
//   k_in_number    a first row's rank is its spelling's id: first-appearance order, no sort
//   k_in_ids       every row takes the id of its slot
#include "fs_internal.h"
#include "fs_dec.h"
#include "fs_probe.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kChunk = 64;                 // bytes per lane: one word of the row-start mask
constexpr uint32_t kTile = kBlock * kChunk;     // bytes per workgroup
constexpr uint32_t kFields = FS_MATCH_FIELDS;
constexpr uint32_t kPad = 128;                  // zero bytes behind the file on the device
constexpr uint32_t kStage = 8192;               // LDS bytes a wave stages its 64 rows in

const char kHeader[] =
    "FAN_WORK_FILENAME,FAN_WORK_WORD_INDEX,FAN_WORK_WORD,FAN_WORK_ORTH_ID,"
    "ORIGINAL_SCRIPT_WORD_INDEX,ORIGINAL_SCRIPT_WORD,ORIGINAL_SCRIPT_ORTH_ID,"
    "ORIGINAL_SCRIPT_CHARACTER,ORIGINAL_SCRIPT_SCENE,BEST_MATCH_DISTANCE,"
    "BEST_LEVENSHTEIN_DISTANCE,BEST_COMBINED_DISTANCE";

// status words on the device
enum { kStBad = 0, kStDefer = 1, kStWords = 4 };

// ---- what one byte may be, given its neighbours and the quoting state in front of it ----

FS_DEC_HD inline bool is_cont(int b) { return b >= 0x80 && b <= 0xBF; }

// FS_MATCH_BAD_UTF8 or 0: c (at i) with the three bytes on either side, -1 outside the file
FS_DEC_HD inline uint32_t utf8_check(int c, int p1, int p2, int p3, int n1, int n2, int n3) {
  if (c < 0x80) return 0;
  bool ok;
  if (c <= 0xBF)
    ok = (p1 >= 0xC2 && p1 <= 0xF4) || (is_cont(p1) && p2 >= 0xE0 && p2 <= 0xF4) ||
         (is_cont(p1) && is_cont(p2) && p3 >= 0xF0 && p3 <= 0xF4);
  else if (c < 0xC2 || c > 0xF4)
    ok = false;
  else if (c < 0xE0)
    ok = is_cont(n1);
  else if (c < 0xF0)
    ok = is_cont(n1) && is_cont(n2) && !(c == 0xE0 && n1 < 0xA0) && !(c == 0xED && n1 > 0x9F);
  else
    ok = is_cont(n1) && is_cont(n2) && is_cont(n3) && !(c == 0xF0 && n1 < 0x90) &&
         !(c == 0xF4 && n1 > 0x8F);
  return ok ? 0 : FS_MATCH_BAD_UTF8;
}

// The conditions on byte c at offset i; q: inside quotes in front of it (updated).  *start: a
// non-empty row starts here.
FS_DEC_HD inline uint32_t byte_check(uint64_t i, int c, int p1, int n1, bool& q, bool* start) {
  uint32_t bad = 0;
  *start = !q && (i == 0 || p1 == '\n') && !(c == '\n' || (c == '\r' && n1 == '\n'));
  if (c == 0) bad |= FS_MATCH_BAD_NUL;
  if (c == '"') {
    if (!q) {
      if (!(i == 0 || p1 == ',' || p1 == '\n' || p1 == '"')) bad |= FS_MATCH_BAD_OPEN;
    } else if (!(n1 < 0 || n1 == ',' || n1 == '\n' || n1 == '\r' || n1 == '"')) {
      bad |= FS_MATCH_BAD_CLOSE;
    }
    q = !q;
  } else if (!q && c == '\r' && n1 != '\n') {
    bad |= FS_MATCH_BAD_CR;
  }
  return bad;
}

// 0x80 in every byte of x that equals '"'
FS_DEC_HD inline uint32_t quote_bytes(uint32_t x) {
  const uint32_t y = x ^ 0x22222222u;
  return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}

// ---- one row ----

struct RowOut {
  uint32_t fan, orig, lev, bad, quoted, head;
  bool defer_dist, defer_comb;
  double dist, comb;
};

// decimal digits [b, e) of the row at s: 1..10 of them, value < 2^32
template <class Src>
FS_DEC_HD inline bool parse_u32(const Src& src, uint64_t s, uint32_t b, uint32_t e, uint32_t* out) {
  if (e <= b || e - b > 10) return false;
  uint64_t v = 0;
  for (uint32_t k = b; k < e; ++k) {
    const int c = src.get(s + k);
    if (c < '0' || c > '9') return false;
    v = v * 10 + (uint64_t)(c - '0');
  }
  *out = (uint32_t)v;
  return v < (1ull << 32);
}

template <class Src>
FS_DEC_HD inline bool parse_f64(const Src& src, uint64_t s, uint32_t b, uint32_t e, double* out) {
  const auto get = [&](uint32_t k) -> int { return src.get(s + b + k); };
  *out = fs_dec_bits(0x7FF8ull << 48);
  return fs_dec_parse(get, e - b, out) == FS_DEC_SURE;
}

// The row that starts at s (prev: the start of the row in front, or s for the first one); the
// field ends go straight to ends[12].
template <class Src>
FS_DEC_HD inline void parse_row(const Src& src, uint64_t s, uint64_t prev, uint32_t* ends,
                                RowOut& o) {
  uint32_t f = 0, quoted = 0, e0 = 0, e3 = 0, e8 = 0, e9 = 0, e10 = 0;
  uint32_t ef = 0, eo = 0;       // ends of fan_ix and orig_ix
  uint64_t i = s, fstart = s, end = s;
  bool q = false;
  o.bad = 0;
  o.defer_dist = o.defer_comb = false;
  for (uint32_t k = 0; k < kFields; ++k) ends[k] = 0;
  for (;; ++i) {
    const int c = src.get(i);
    if (c < 0) {                               // a last row without a terminator
      if (q) o.bad |= FS_MATCH_BAD_CLOSE;
      end = i;
      break;
    }
    if (c == '"') {
      if (i == fstart && f < kFields) quoted |= 1u << f;
      q = !q;
    } else if (!q) {
      if (c == ',') {
        const uint32_t v = (uint32_t)(i - s);
        if (f < kFields) ends[f] = v;
        if (f == 0) e0 = v;
        else if (f == 1) ef = v;
        else if (f == 3) e3 = v;
        else if (f == 4) eo = v;
        else if (f == 8) e8 = v;
        else if (f == 9) e9 = v;
        else if (f == 10) e10 = v;
        ++f;
        fstart = i + 1;
      } else if (c == '\n' || (c == '\r' && src.get(i + 1) == '\n')) {
        end = i;
        break;
      }
    }
  }
  if (end - s >= (1ull << 32)) {
    o.bad |= FS_MATCH_BAD_ROW;
    return;
  }
  const uint32_t e11 = (uint32_t)(end - s);
  if (f != kFields - 1) {
    o.bad |= FS_MATCH_BAD_FIELDS;
    return;
  }
  ends[kFields - 1] = e11;
  o.quoted = quoted;
  if (!parse_u32(src, s, e0 + 1, ef, &o.fan) || !parse_u32(src, s, e3 + 1, eo, &o.orig) ||
      !parse_u32(src, s, e9 + 1, e10, &o.lev)) {
    o.bad |= FS_MATCH_BAD_INT;
    return;
  }
  o.defer_dist = !parse_f64(src, s, e8 + 1, e9, &o.dist);
  o.defer_comb = !parse_f64(src, s, e10 + 1, e11, &o.comb);
  // equal bytes up to and with the comma behind the name: the same field, ended alike
  bool head = prev == s;
  for (uint32_t k = 0; k <= e0 && !head; ++k) head = src.get(prev + k) != src.get(s + k);
  o.head = head ? 1u : 0u;
}

// the file's bytes where they lie
struct GlobalSrc {
  const uint8_t* d;
  uint64_t n;
  FS_DEC_HD int get(uint64_t i) const { return i < n ? (int)d[i] : -1; }
};

// ... and the stretch [lo, lo + len) of them copied to LDS
struct StagedSrc {
  const uint8_t* d;
  uint64_t n;
  const uint8_t* s;
  uint64_t lo;
  uint32_t len;
  __device__ int get(uint64_t i) const {
    if (i >= n) return -1;
    const uint64_t k = i - lo;
    return k < len ? (int)s[k] : (int)d[i];
  }
};

// ---- kernels ----

__global__ __launch_bounds__(kBlock) void k_mt_parity(const uint8_t* __restrict__ d, uint64_t n,
                                                      uint32_t* __restrict__ par) {
  __shared__ uint32_t s_par;
  if (threadIdx.x == 0) s_par = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kChunk;
  uint32_t cnt = 0;
  if (base < n) {                                // the padding behind n holds no quote
    const uint4* p = reinterpret_cast<const uint4*>(d + base);
#pragma unroll
    for (uint32_t k = 0; k < kChunk / 16; ++k) {
      const uint4 v = p[k];
      cnt += __popc(quote_bytes(v.x)) + __popc(quote_bytes(v.y)) + __popc(quote_bytes(v.z)) +
             __popc(quote_bytes(v.w));
    }
  }
  const uint64_t b = __ballot(cnt & 1);
  if ((threadIdx.x & 63) == 0) atomicXor(&s_par, (uint32_t)__popcll(b) & 1u);
  __syncthreads();
  if (threadIdx.x == 0) par[blockIdx.x] = s_par;
}

// exclusive scan of v[0..nb) in place, *total = sum (one workgroup, chunks of 1024 in turn)
// (the 32-bit prefixes are used only when the total fits)
__global__ __launch_bounds__(kScanBlock) void k_mt_scan(uint32_t* v, uint32_t nb,
                                                        uint64_t* __restrict__ total) {
  scan_array<uint32_t, uint64_t>(v, nb, v, total);
}

__global__ __launch_bounds__(kBlock) void k_mt_classify(const uint8_t* __restrict__ d, uint64_t n,
                                                        const uint32_t* __restrict__ par,
                                                        uint64_t* __restrict__ mask,
                                                        uint32_t* __restrict__ cnt,
                                                        uint32_t* __restrict__ status) {
  __shared__ uint32_t s_wpar[kBlock / 64];
  __shared__ uint32_t s_cnt;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * kChunk;
  if (threadIdx.x == 0) s_cnt = 0;
  uint64_t x[kChunk / 8 + 1];                    // the lane's bytes and the three behind them
  uint32_t quotes = 0;
  const bool live = base < n;
  if (live) {
    const uint4* p = reinterpret_cast<const uint4*>(d + base);
#pragma unroll
    for (uint32_t k = 0; k < kChunk / 16; ++k) {
      const uint4 v = p[k];
      quotes += __popc(quote_bytes(v.x)) + __popc(quote_bytes(v.y)) + __popc(quote_bytes(v.z)) +
                __popc(quote_bytes(v.w));
      x[2 * k] = (uint64_t)v.x | (uint64_t)v.y << 32;
      x[2 * k + 1] = (uint64_t)v.z | (uint64_t)v.w << 32;
    }
    const uint8_t* t = d + base + kChunk;        // (inside the padding where the file ends)
    x[kChunk / 8] = (uint64_t)t[0] | (uint64_t)t[1] << 8 | (uint64_t)t[2] << 16;
  }
  const uint64_t b = __ballot(quotes & 1);
  if (lane == 0) s_wpar[wave] = (uint32_t)__popcll(b) & 1u;
  __syncthreads();
  uint32_t p0 = par[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1));
  for (uint32_t k = 0; k < wave; ++k) p0 += s_wpar[k];
  uint64_t starts = 0;
  uint32_t bad = 0;
  if (live) {
    bool q = p0 & 1;
    const auto before = [&](uint64_t k) -> int { return base >= k ? (int)d[base - k] : -1; };
    int p3 = before(3), p2 = before(2), p1 = before(1);
    // the bytes pass through x[0]'s low end, so that no register is picked by a run-time index
#pragma unroll 1
    for (uint32_t j = 0; j < kChunk; ++j) {
      const uint64_t i = base + j;
      if (i >= n) break;
      const int c = (int)(x[0] & 0xFF);
      const int n1 = i + 1 < n ? (int)((x[0] >> 8) & 0xFF) : -1;
      const int n2 = i + 2 < n ? (int)((x[0] >> 16) & 0xFF) : -1;
      const int n3 = i + 3 < n ? (int)((x[0] >> 24) & 0xFF) : -1;
      bool start;
      bad |= byte_check(i, c, p1, n1, q, &start);
      bad |= utf8_check(c, p1, p2, p3, n1, n2, n3);
      if (start) starts |= 1ull << j;
      if (i + 1 == n && q) bad |= FS_MATCH_BAD_CLOSE;   // the file ends inside quotes
      p3 = p2, p2 = p1, p1 = c;
#pragma unroll
      for (uint32_t k = 0; k < kChunk / 8; ++k) x[k] = x[k] >> 8 | x[k + 1] << 56;
      x[kChunk / 8] >>= 8;
    }
    mask[base / kChunk] = starts;
  }
  if (starts) atomicAdd(&s_cnt, (uint32_t)__popcll(starts));
  if (bad) atomicOr(&status[kStBad], bad);
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = s_cnt;
}

// row_start[k] = offset of the first byte of non-empty row k
__global__ __launch_bounds__(kBlock) void k_mt_place(const uint64_t* __restrict__ mask,
                                                     uint64_t n_words,
                                                     const uint32_t* __restrict__ off,
                                                     uint64_t* __restrict__ row_start) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t word = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint64_t m = word < n_words ? mask[word] : 0;
  const uint32_t c = (uint32_t)__popcll(m);
  const uint32_t inc = wave_scan(c);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  uint64_t pos = (uint64_t)off[blockIdx.x] + inc - c;
  for (uint32_t k = 0; k < wave; ++k) pos += s_w[k];
  for (; m; m &= m - 1) row_start[pos++] = word * kChunk + (uint32_t)__builtin_ctzll(m);
}

struct RowsArgs {
  const uint8_t* d;
  uint64_t n;
  const uint64_t* row_start;     // of all non-empty rows, the header too
  uint64_t n_all;                // their number
  uint32_t first;                // 1: row 0 is the header
  uint32_t n_rows;               // records = n_all - first
  uint32_t* fan;
  uint32_t* orig;
  uint32_t* lev;
  double* dist;
  double* comb;
  fs_match_ix* ix;
  fs_match_defer* defer;
  uint32_t defer_cap;
  uint32_t* status;
};

constexpr uint32_t kColDist = 9, kColComb = 11;

__device__ inline void row_defer(const RowsArgs& a, uint32_t r, uint32_t col) {
  const uint32_t slot = atomicAdd(&a.status[kStDefer], 1u);
  if (slot < a.defer_cap) a.defer[slot] = fs_match_defer{r, col};
}

__device__ inline void row_store(const RowsArgs& a, uint32_t r, uint64_t s, const RowOut& o) {
  if (o.bad) {
    atomicOr(&a.status[kStBad], o.bad);
    return;
  }
  a.fan[r] = o.fan;
  a.orig[r] = o.orig;
  a.lev[r] = o.lev;
  a.dist[r] = o.dist;
  a.comb[r] = o.comb;
  a.ix[r].start = s;
  a.ix[r].quoted = o.quoted;
  a.ix[r].head = o.head;
  if (o.defer_dist) row_defer(a, r, kColDist);
  if (o.defer_comb) row_defer(a, r, kColComb);
}

template <bool kStaged>
__global__ __launch_bounds__(kBlock) void k_mt_rows(RowsArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_bytes[kStaged ? kBlock / 64 * kStage : 16];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  const bool live = r < a.n_rows;
  const uint64_t R = (uint64_t)r + a.first;
  const uint64_t s = live ? a.row_start[R] : 0;
  const uint64_t prev = live && r > 0 ? a.row_start[R - 1] : s;
  RowOut o;
  if (kStaged) {
    // the wave's rows and the one in front: [lo, hi), read 16 bytes a lane at a time
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r0 = r - lane;                            // wave-uniform
    uint8_t* mine = s_bytes + wave * kStage;
    uint64_t lo = 0, len = 0;
    if (r0 < a.n_rows) {
      const uint64_t R0 = (uint64_t)r0 + a.first;
      lo = a.row_start[r0 > 0 ? R0 - 1 : R0] & ~15ull;
      const uint64_t hi = R0 + 64 < a.n_all ? a.row_start[R0 + 64] : a.n;
      len = hi - lo <= kStage ? hi - lo : 0;                 // too long: read where they lie
      for (uint64_t k = (uint64_t)lane * 16; k < len; k += 64 * 16)   // (kPad covers the last 16)
        *reinterpret_cast<uint4*>(mine + k) = *reinterpret_cast<const uint4*>(a.d + lo + k);
    }
    __syncthreads();
    if (!live) return;
    parse_row(StagedSrc{a.d, a.n, mine, lo, (uint32_t)len}, s, prev, a.ix[r].end, o);
  } else {
    if (!live) return;
    parse_row(GlobalSrc{a.d, a.n}, s, prev, a.ix[r].end, o);
  }
  row_store(a, r, s, o);
}

// first[w] = smallest record that names script word w
__global__ __launch_bounds__(kBlock) void k_mt_first(const uint32_t* __restrict__ orig, uint32_t n,
                                                     uint32_t n_script, uint32_t* __restrict__ first,
                                                     uint32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t w = orig[i];
  if (w >= n_script)
    atomicOr(&status[kStBad], 1u);
  else
    atomicMin(&first[w], i);
}

// records whose field `col` differs in its bytes from that of first[their script word]
__global__ __launch_bounds__(kBlock) void k_mt_differ(const uint8_t* __restrict__ d,
                                                      const fs_match_ix* __restrict__ ix,
                                                      const uint32_t* __restrict__ orig, uint32_t n,
                                                      uint32_t col,
                                                      const uint32_t* __restrict__ first,
                                                      unsigned long long* __restrict__ n_differ) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  bool differ = false;
  if (i < n) {
    const uint32_t j = first[orig[i]];
    if (j != i) {
      const uint32_t bi = col ? ix[i].end[col - 1] + 1 : 0, ei = ix[i].end[col];
      const uint32_t bj = col ? ix[j].end[col - 1] + 1 : 0, ej = ix[j].end[col];
      differ = ei - bi != ej - bj;
      const uint8_t* pi = d + ix[i].start + bi;
      const uint8_t* pj = d + ix[j].start + bj;
      for (uint32_t k = 0; k < ei - bi && !differ; ++k) differ = pi[k] != pj[k];
    }
  }
  const uint64_t b = __ballot(differ);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_differ, (unsigned long long)__popcll(b));
}

// ---- interning a text column ----

struct InternArgs {
  const uint8_t* d;
  const fs_match_ix* ix;
  uint32_t n, col;
  uint64_t mask;                 // slots - 1
  uint64_t hash_mask;            // FS_INTERN_HASH_BITS: the bits of the hash that are kept
  unsigned long long* slots;     // {tag << 32 | row that claimed the slot}
  uint32_t* first;               // [slots] smallest row of the slot's spelling
  uint32_t* slot_of;             // [n]
  uint32_t* slot_id;             // [slots] id of the slot's spelling
  uint32_t* cnt;                 // [blocks] first rows per block, then their exclusive scan
  uint32_t* list;                // [n_distinct] first rows, ascending
  uint32_t* id;                  // [n]
};

// where field `col` of row r lies: any offset, any length
__device__ inline const uint8_t* intern_field(const InternArgs& a, uint32_t r, uint32_t* len) {
  const fs_match_ix* __restrict__ x = a.ix + r;
  const uint32_t b = a.col ? x->end[a.col - 1] + 1 : 0;
  *len = x->end[a.col] - b;
  return a.d + x->start + b;
}

__global__ __launch_bounds__(kBlock) void k_in_insert(InternArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= a.n) return;
  uint32_t len;
  const uint8_t* __restrict__ p = intern_field(a, r, &len);
  uint64_t h = 0xCBF29CE484222325ull;                       // FNV-1a over the bytes
  for (uint32_t k = 0; k < len; ++k) h = (h ^ p[k]) * 0x100000001B3ull;
  h = fs_mix64(fs_mix64(h ^ len) & a.hash_mask);            // the kept bits decide slot and tag
  const uint32_t tag = (uint32_t)(h >> 32);
  const auto same = [&](unsigned long long cur) -> bool {
    if ((uint32_t)(cur >> 32) != tag) return false;
    uint32_t lj;
    const uint8_t* __restrict__ q = intern_field(a, (uint32_t)cur, &lj);
    if (lj != len) return false;
    for (uint32_t k = 0; k < len; ++k)
      if (p[k] != q[k]) return false;
    return true;
  };
  bool inserted;
  const uint64_t slot = fs_probe_insert(a.slots, a.mask, h, (unsigned long long)tag << 32 | r,
                                        same, &inserted);
  a.slot_of[r] = (uint32_t)slot;
  // a value read here is never below the slot's final one: a row at or above it need not try
  if (r < __hip_atomic_load(&a.first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(&a.first[slot], r);
}

// this row is the first of its spelling; its rank among such rows of the workgroup in *rank,
// their number in *total
__device__ inline bool intern_head(const InternArgs& a, uint32_t* rank, uint32_t* total) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  const bool head = r < a.n && a.first[a.slot_of[r]] == r;
  block_rank<kBlock>(head, s_w, rank, total);
  return head;
}

__global__ __launch_bounds__(kBlock) void k_in_count(InternArgs a) {
  uint32_t rank, total;
  intern_head(a, &rank, &total);
  if (threadIdx.x == 0) a.cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void k_in_number(InternArgs a) {
  uint32_t rank, total;
  if (!intern_head(a, &rank, &total)) return;
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t k = a.cnt[blockIdx.x] + rank;
  a.slot_id[a.slot_of[r]] = k;
  a.list[k] = r;
}

__global__ __launch_bounds__(kBlock) void k_in_ids(InternArgs a) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < a.n) a.id[r] = a.slot_id[a.slot_of[r]];
}

uint64_t intern_hash_mask() {
  const char* e = getenv("FS_INTERN_HASH_BITS");   // diagnostic: k bits of the hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1;
}

uint32_t tiles(uint64_t n_bytes) { return (uint32_t)((n_bytes + kTile - 1) / kTile); }

bool staged_default() {
  const char* e = getenv("FS_MATCHES_STAGE");     // 0: every lane reads global memory
  return !(e && e[0] == '0');
}

// the header row at bytes[at ..), ended by a terminator or the end of the file
bool is_header(const uint8_t* bytes, uint64_t n, uint64_t at) {
  const uint64_t len = sizeof kHeader - 1;
  if (n - at < len || memcmp(bytes + at, kHeader, len) != 0) return false;
  const uint64_t e = at + len;
  return e == n || bytes[e] == '\n' || (e + 1 < n && bytes[e] == '\r' && bytes[e + 1] == '\n');
}

}  // namespace

struct fs_matches {
  int device = 0;
  uint64_t n_bytes = 0;
  fs_matches_info info{};
  DBuf<uint8_t> bytes;
  DBuf<uint32_t> par, cnt, status, fan, orig, lev, first;
  DBuf<uint64_t> mask, row_start, total;
  DBuf<double> dist, comb;
  DBuf<fs_match_ix> ix;
  DBuf<fs_match_defer> defer;
  uint32_t defer_cap = 0;
  // fs_matches_intern
  DBuf<unsigned long long> in_slots;
  DBuf<uint32_t> in_first, in_slot_of, in_slot_id, in_cnt, in_list, in_id;
  double in_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

int matches_run(fs_matches* m, const uint8_t* bytes, uint64_t n) {
  fs_matches_info& info = m->info;
  Clock<7> clk;
  const uint32_t nb = tiles(n);
  const uint64_t n_words = (n + kChunk - 1) / kChunk;
  FS_TRY(m->bytes.reserve(n + kPad));
  FS_TRY(m->par.reserve(nb));
  FS_TRY(m->cnt.reserve(nb));
  FS_TRY(m->mask.reserve(n_words));
  FS_TRY(m->status.reserve(kStWords));
  FS_TRY(m->total.reserve(2));
  FS_TRY(clk.mark(0, nullptr));
  FS_HIP(hipMemcpyAsync(m->bytes.p, bytes, n, hipMemcpyHostToDevice, nullptr));
  FS_HIP(hipMemsetAsync(m->bytes.p + n, 0, kPad, nullptr));
  FS_HIP(hipMemsetAsync(m->status.p, 0, kStWords * sizeof(uint32_t), nullptr));
  FS_TRY(clk.mark(1, nullptr));
  hipLaunchKernelGGL(k_mt_parity, dim3(nb), dim3(kBlock), 0, nullptr, m->bytes.p, n, m->par.p);
  hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(kScanBlock), 0, nullptr, m->par.p, nb, m->total.p);
  FS_TRY(clk.mark(2, nullptr));
  hipLaunchKernelGGL(k_mt_classify, dim3(nb), dim3(kBlock), 0, nullptr, m->bytes.p, n, m->par.p,
                     m->mask.p, m->cnt.p, m->status.p);
  FS_TRY(clk.mark(3, nullptr));
  hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(kScanBlock), 0, nullptr, m->cnt.p, nb,
                     m->total.p + 1);
  FS_HIP(hipGetLastError());
  uint32_t st[kStWords];
  uint64_t total[2];
  FS_HIP(hipMemcpyAsync(st, m->status.p, sizeof st, hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(total, m->total.p, sizeof total, hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipStreamSynchronize(nullptr));
  const auto timings = [&](int last) {
    for (int k = 0; k < last; ++k) info.ms[k] = clk.elapsed(k, k + 1);
    info.ms[6] = clk.elapsed(0, last);
  };
  if (st[kStBad]) {
    info.status = FS_MATCHES_OUTSIDE;
    info.reason = st[kStBad];
    timings(3);
    return FS_OK;
  }
  const uint64_t n_all = total[1];
  if (n_all == 0) {
    timings(3);
    return FS_OK;
  }
  FS_TRY(m->row_start.reserve(n_all));
  hipLaunchKernelGGL(k_mt_place, dim3(nb), dim3(kBlock), 0, nullptr, m->mask.p, n_words, m->cnt.p,
                     m->row_start.p);
  FS_TRY(clk.mark(4, nullptr));
  uint64_t start0 = 0;
  FS_HIP(hipMemcpy(&start0, m->row_start.p, sizeof start0, hipMemcpyDeviceToHost));
  info.has_header = is_header(bytes, n, start0) ? 1u : 0u;
  const uint64_t n_rows = n_all - info.has_header;
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: the reader takes fewer than 2^32", (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  if (n_rows == 0) {
    timings(4);
    return FS_OK;
  }
  FS_TRY(m->fan.reserve(n_rows));
  FS_TRY(m->orig.reserve(n_rows));
  FS_TRY(m->lev.reserve(n_rows));
  FS_TRY(m->dist.reserve(n_rows));
  FS_TRY(m->comb.reserve(n_rows));
  FS_TRY(m->ix.reserve(n_rows));
  m->defer_cap = (uint32_t)(n_rows / 16 < 4096 ? 4096 : n_rows / 16);
  FS_TRY(m->defer.reserve(m->defer_cap));
  const RowsArgs a{m->bytes.p, n, m->row_start.p, n_all, info.has_header, (uint32_t)n_rows,
                   m->fan.p, m->orig.p, m->lev.p, m->dist.p, m->comb.p, m->ix.p, m->defer.p,
                   m->defer_cap, m->status.p};
  const dim3 grid((uint32_t)((n_rows + kBlock - 1) / kBlock));
  FS_TRY(clk.mark(5, nullptr));
  if (staged_default())
    hipLaunchKernelGGL(k_mt_rows<true>, grid, dim3(kBlock), 0, nullptr, a);
  else
    hipLaunchKernelGGL(k_mt_rows<false>, grid, dim3(kBlock), 0, nullptr, a);
  FS_TRY(clk.mark(6, nullptr));
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, m->status.p, sizeof st, hipMemcpyDeviceToHost));
  timings(6);
  if (st[kStBad] || st[kStDefer] > m->defer_cap) {
    // more fields left over than a writer's file ever has: not this reader's file either
    info.status = FS_MATCHES_OUTSIDE;
    info.reason = st[kStBad] ? st[kStBad] : (uint32_t)FS_MATCH_BAD_DEFER;
    return FS_OK;
  }
  info.n_rows = n_rows;
  info.n_deferred = st[kStDefer];
  info.status = st[kStDefer] ? FS_MATCHES_DEFERRED : FS_MATCHES_PARSED;
  return FS_OK;
}

}  // namespace

extern "C" int fs_matches_open(int device, const uint8_t* bytes, uint64_t n_bytes,
                               fs_matches** out, fs_matches_info* info) {
  if (!out || !info || (n_bytes && !bytes)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  *out = nullptr;
  fs_matches* m = new fs_matches;
  m->device = device;
  m->n_bytes = n_bytes;
  m->info.status = FS_MATCHES_PARSED;
  const uint64_t hl = sizeof kHeader - 1;
  // nothing, or the header alone: no device work
  const bool header_only = n_bytes >= hl && n_bytes <= hl + 2 && is_header(bytes, n_bytes, 0) &&
                           (n_bytes == hl || bytes[n_bytes - 1] == '\n');
  int rc = FS_OK;
  if (header_only) {
    m->info.has_header = 1;
  } else if (n_bytes) {
    hipError_t e = hipSetDevice(device);
    (void)hipGetLastError();
    if (e != hipSuccess) {
      fs_set_error("hipSetDevice(%d) -> %s", device, hipGetErrorString(e));
      rc = FS_E_DEVICE;
    } else {
      rc = matches_run(m, bytes, n_bytes);
    }
  }
  if (rc != FS_OK) {
    delete m;
    return rc;
  }
  *info = m->info;
  *out = m;
  return FS_OK;
}

extern "C" int fs_matches_read(fs_matches* m, uint32_t* fan_ix, uint32_t* orig_ix, uint32_t* lev,
                               double* dist, double* comb, fs_match_ix* ix, uint64_t cap,
                               fs_match_defer* deferred, uint64_t defer_cap) {
  if (!m) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (m->info.status == FS_MATCHES_OUTSIDE) {
    fs_set_error("the file is outside the reader's grammar: nothing to read");
    return FS_E_INVALID;
  }
  const uint64_t n = m->info.n_rows, nd = m->info.n_deferred;
  if (cap < n || defer_cap < nd) {
    fs_set_error("%llu rows and %llu deferred fields need room", (unsigned long long)n,
                 (unsigned long long)nd);
    return FS_E_CAPACITY;
  }
  if (!n) return FS_OK;
  if (!fan_ix || !orig_ix || !lev || !dist || !comb || !ix || (nd && !deferred)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(m->device);
  FS_HIP(hipMemcpyAsync(fan_ix, m->fan.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(orig_ix, m->orig.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(lev, m->lev.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(dist, m->dist.p, n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(comb, m->comb.p, n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(ix, m->ix.p, n * sizeof(fs_match_ix), hipMemcpyDeviceToHost, nullptr));
  if (nd)
    FS_HIP(hipMemcpyAsync(deferred, m->defer.p, nd * sizeof(fs_match_defer),
                          hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipStreamSynchronize(nullptr));
  return FS_OK;
}

extern "C" int fs_matches_labels(fs_matches* m, uint32_t column, uint32_t n_script,
                                 uint32_t* first, uint64_t* n_differ) {
  if (!m || !n_differ || (n_script && !first)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (m->info.status == FS_MATCHES_OUTSIDE || column >= kFields) {
    fs_set_error("no parsed file, or column %u of %u", column, kFields);
    return FS_E_INVALID;
  }
  *n_differ = 0;
  for (uint32_t w = 0; w < n_script; ++w) first[w] = 0xFFFFFFFFu;
  const uint32_t n = (uint32_t)m->info.n_rows;
  if (!n) return FS_OK;
  FS_ENTER(m->device);
  FS_TRY(m->first.reserve(n_script));
  FS_HIP(hipMemsetAsync(m->first.p, 0xFF, (size_t)n_script * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(m->status.p, 0, kStWords * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(m->total.p, 0, sizeof(uint64_t), nullptr));
  const dim3 grid((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_mt_first, grid, dim3(kBlock), 0, nullptr, m->orig.p, n, n_script,
                     m->first.p, m->status.p);
  FS_HIP(hipGetLastError());
  uint32_t bad = 0;
  FS_HIP(hipMemcpy(&bad, m->status.p, sizeof bad, hipMemcpyDeviceToHost));
  if (bad) {
    fs_set_error("a record names a script word beyond n_script = %u", n_script);
    return FS_E_INVALID;
  }
  hipLaunchKernelGGL(k_mt_differ, grid, dim3(kBlock), 0, nullptr, m->bytes.p, m->ix.p, m->orig.p,
                     n, column, m->first.p,
                     reinterpret_cast<unsigned long long*>(m->total.p));
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(first, m->first.p, (size_t)n_script * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(n_differ, m->total.p, sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipStreamSynchronize(nullptr));
  return FS_OK;
}

extern "C" int fs_matches_intern(fs_matches* m, uint32_t column, uint32_t* id, uint32_t* first,
                                 uint64_t cap, uint64_t* n_distinct) {
  if (!m || !n_distinct) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (m->info.status == FS_MATCHES_OUTSIDE || column >= kFields) {
    fs_set_error("no parsed file, or column %u of %u", column, kFields);
    return FS_E_INVALID;
  }
  *n_distinct = 0;
  for (double& t : m->in_ms) t = 0.0;
  const uint32_t n = (uint32_t)m->info.n_rows;
  if (!n) return FS_OK;
  if (!id || (cap && !first)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(m->device);
  Clock<5> clk;
  uint64_t slots = fs_probe_slots(n);
  if (slots > (1ull << 32)) slots = 1ull << 32;              // (slot numbers are 32 bits)
  const uint32_t blocks = blocks_of(n, kBlock);
  FS_TRY(m->in_slots.reserve(slots));
  FS_TRY(m->in_first.reserve(slots));
  FS_TRY(m->in_slot_id.reserve(slots));
  FS_TRY(m->in_slot_of.reserve(n));
  FS_TRY(m->in_id.reserve(n));
  FS_TRY(m->in_cnt.reserve(blocks));
  InternArgs a{};
  a.d = m->bytes.p;
  a.ix = m->ix.p;
  a.n = n;
  a.col = column;
  a.mask = slots - 1;
  a.hash_mask = intern_hash_mask();
  a.slots = m->in_slots.p;
  a.first = m->in_first.p;
  a.slot_of = m->in_slot_of.p;
  a.slot_id = m->in_slot_id.p;
  a.cnt = m->in_cnt.p;
  a.id = m->in_id.p;
  FS_TRY(clk.mark(0, nullptr));
  FS_HIP(hipMemsetAsync(a.slots, 0xFF, slots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(a.first, 0xFF, slots * sizeof(uint32_t), nullptr));
  FS_TRY(clk.mark(1, nullptr));
  hipLaunchKernelGGL(k_in_insert, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  FS_TRY(clk.mark(2, nullptr));
  hipLaunchKernelGGL(k_in_count, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_mt_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.cnt, blocks, m->total.p);
  FS_HIP(hipGetLastError());
  uint64_t total = 0;
  FS_HIP(hipMemcpy(&total, m->total.p, sizeof total, hipMemcpyDeviceToHost));
  FS_TRY(m->in_list.reserve(total));
  a.list = m->in_list.p;
  hipLaunchKernelGGL(k_in_number, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_in_ids, dim3(blocks), dim3(kBlock), 0, nullptr, a);
  FS_TRY(clk.mark(3, nullptr));
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(id, a.id, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  if (total <= cap)
    FS_HIP(hipMemcpyAsync(first, a.list, total * sizeof(uint32_t), hipMemcpyDeviceToHost, nullptr));
  FS_TRY(clk.mark(4, nullptr));
  FS_HIP(hipStreamSynchronize(nullptr));
  for (int k = 0; k < 4; ++k) m->in_ms[k] = clk.elapsed(k, k + 1);
  m->in_ms[4] = clk.elapsed(0, 4);
  *n_distinct = total;
  if (total > cap) {
    fs_set_error("%llu spellings need room", (unsigned long long)total);
    return FS_E_CAPACITY;
  }
  return FS_OK;
}

extern "C" int fs_matches_intern_times(const fs_matches* m, double* ms) {
  if (!m || !ms) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  for (int k = 0; k < 8; ++k) ms[k] = m->in_ms[k];
  return FS_OK;
}

extern "C" void fs_matches_close(fs_matches* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  delete m;
}

extern "C" int fs_matches_parse_double(const uint8_t* bytes, uint64_t len, double* out) {
  if (!out || (len && !bytes) || len > 0xFFFFFFFFull) return FS_DEC_NOT_MINE;
  const auto get = [bytes](uint32_t i) -> int { return bytes[i]; };
  return fs_dec_parse(get, (uint32_t)len, out);
}
