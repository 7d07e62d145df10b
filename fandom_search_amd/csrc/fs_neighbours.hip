// fs_neighbours.hip -- `ao3.py neighbours`: each fan work's closest works by the rare script words
// both quote (fs_neighbours, fs_neighbours_rows in include/fandom_search.h).  The coverage of a
// work is a row of bits over the script, as in fs_pairs.hip; a script word weighs the more the
// fewer works cover it, and the score of two works is the sum of the weights of the words in both
// rows: one product of the 0/1 bytes of one row and the weight bytes under the bits of the other.
//
// Every output is an integer, and a list is the K largest of a set of distinct 64-bit keys, so
// partial results merge in any order.  Separate launches; no workgroup waits on another:
//   CoverJob         number / reserve / cover of fs_tiles.h: the matrix, the active numbering
//   k_nb_depth       the column counts of the matrix: a wave takes the word k of 64 rows and
//                    turns it by 64 ballots, lane j the count of bit j; one atomic add per lane.
//                    It also notes, a bit per (tile, k), the words k in which a tile has a bit
//   k_nb_weight      a lane per script word: its weight byte (zeros up to nk * 64), its
//                    fs_neighbour_word
//   k_nb_own         a lane per row: own(a), the weights under its bits (a row pass, not the
//                    product's diagonal: the diagonal tile is one of many a stripe walks)
//   k_nb_product<1>  the hot path: v_mfma_i32_16x16x64_i8 with the fragment maps at the head of
//                    fs_intervals.hip.  A workgroup owns a stripe of 64 rows and a share of the
//                    column tiles; each of its four waves takes every fourth column tile of the
//                    share whole, 64 x 64 scores: per 64-bit word k four row fragments expanded
//                    to 0/1 bytes and four column fragments expanded and masked with the sixteen
//                    weight bytes of the lane's bits, eight expansions for sixteen MFMAs; only
//                    the words k in which both tiles have a bit are walked.  The scores stay in
//                    registers: the candidate rule and the test against the row's K-th key are
//                    two 64-bit multiplications and no division; the few that pass are divided
//                    and inserted, the wave together, into the wave's own sorted list of the row
//                    in LDS.  The wave's lists and candidate counts go out as one of the row's
//                    partial lists
//   k_nb_product<0>  FS_NEIGHBOURS_MFMA=0: the same with the scores of a tile from the AND of two
//                    words and a walk of its set bits; no matrix instruction
//   k_nb_merge       a wave per row: the partial lists into one, a slot a lane; the counts added
//   k_nb_back        a lane per list slot: the back rank by a look through the partner's list;
//                    LISTED_BY and MUTUAL by atomic adds (here and not in the detail pass: the
//                    works table is complete when the listed pairs do not fit)
//   k_pairs_scan     the offsets of the lists
//   k_nb_works       a lane per work: its fs_neighbour_work
//   k_nb_place       a lane per list slot: the listed pair's head in (work, rank) order
//   k_nb_detail      a lane per listed pair: the AND of the two rows walked once for the shared
//                    words, the score and the rarest word, then the run around it
#include "fs_tiles.h"

namespace {

constexpr uint32_t kProd = 256;               // threads of k_nb_product: four waves
constexpr uint32_t kWaves = kProd / 64;
constexpr uint32_t kFr = kTile / 16;          // fragments of 16 rows (columns) in a tile
constexpr uint32_t kMaxTop = FS_NEIGHBOURS_MAX_TOP;
constexpr uint32_t kSplitBlocks = 512;        // below this many stripes the column tiles are
constexpr uint32_t kSplitTiles = kWaves;      // shared out, at least a tile a wave to each share
constexpr uint32_t kMfmaDefault = 1u;         // FS_NEIGHBOURS_MFMA unset
constexpr uint64_t kMillion = 1000000ull;

typedef int v4i __attribute__((ext_vector_type(4)));

struct NbArgs : CoverArgs {
  uint32_t K;                   // top
  uint32_t flat;                // 1: every covered word weighs 1
  uint32_t min_score, min_ppm;
  uint32_t S, P;                // shares of the column tiles; partial lists of a row: S * kWaves
  uint32_t nkw;                 // 64-bit words of a tile's row of `some`: ceil(nk / 64)
  uint32_t* depth;              // [nk * 64]
  unsigned long long* some;     // [n_tiles][nkw] bit k: a row of the tile has a bit in word k
  uint8_t* wb;                  // [nk * 64] weight bytes
  uint32_t* own;                // [n_tiles * 64]
  unsigned long long* part;     // [n_tiles * 64][P][K] sorted, larger first, 0: empty
  uint32_t* pcand;              // [n_tiles * 64][P]
  unsigned long long* lists;    // [n_tiles * 64][K]
  uint32_t* back;               // [n_tiles * 64][K]
  uint32_t* cand;               // [n_tiles * 64]
  uint32_t* listed;             // [n_tiles * 64]
  uint32_t* listed_by;          // [n_tiles * 64]
  uint32_t* mutual;             // [n_tiles * 64]
  unsigned long long* off;      // [n_tiles * 64] listed, scanned
  unsigned long long* total;
  fs_neighbour_work* works;
  fs_neighbour_word* words;
  fs_neighbour* out;
};

// blockIdx.x = word k, the waves of blockIdx.y share the tiles
__global__ __launch_bounds__(kRunBlock) void k_nb_depth(NbArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t k = blockIdx.x;
  const uint32_t step = gridDim.y * (kRunBlock / 64);
  uint32_t acc = 0;
  for (uint32_t t = blockIdx.y * (kRunBlock / 64) + (threadIdx.x >> 6); t < a.n_tiles; t += step) {
    const unsigned long long x = a.cov[((size_t)t * a.nk + k) * kTile + lane];
    if (!__ballot(x != 0)) continue;
    if (lane == 0) atomicOr(&a.some[(size_t)t * a.nkw + k / 64], 1ull << (k % 64));
    for (uint32_t j = 0; j < 64; ++j) {
      const uint32_t c = (uint32_t)__popcll(__ballot((x >> j) & 1ull));
      if (lane == j) acc += c;
    }
  }
  if (acc) atomicAdd(&a.depth[(size_t)k * 64 + lane], acc);
}

// a lane per script word, the padding up to nk * 64 included
__global__ __launch_bounds__(kRunBlock) void k_nb_weight(NbArgs a) {
  const uint32_t o = blockIdx.x * kRunBlock + threadIdx.x;
  if (o >= a.nk * 64) return;
  const uint32_t d = a.depth[o];
  const uint32_t w = !d ? 0u : a.flat ? 1u : 32u - (uint32_t)__builtin_clz(a.n_active / d);
  a.wb[o] = (uint8_t)w;
  if (o < a.n_script) reinterpret_cast<uint2*>(a.words)[o] = make_uint2(d, w);
}

// a workgroup of 64 lanes per tile: lane r sums the weights under the bits of row r
__global__ __launch_bounds__(kTile) void k_nb_own(NbArgs a) {
  const unsigned long long* t = a.cov + (size_t)blockIdx.x * a.nk * kTile + threadIdx.x;
  uint32_t c = 0;
  for (uint32_t k = 0; k < a.nk; ++k) {
    unsigned long long x = t[(size_t)k * kTile];
    while (x) {
      c += a.wb[k * 64 + (uint32_t)__builtin_ctzll(x)];
      x &= x - 1;
    }
  }
  a.own[(size_t)blockIdx.x * kTile + threadIdx.x] = c;
}

// sixteen bits to sixteen bytes of 0 / 1: bit i of a nibble lands in byte i
__device__ inline v4i spread16(uint32_t x) {
  v4i f;
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d)
    f[d] = (int)((((x >> (4 * d)) & 0xFu) * 0x00204081u) & 0x01010101u);
  return f;
}

// `key` into a list of K distinct keys sorted larger first (0: empty), by the whole wave: slot
// `lane` is lane's
__device__ inline void nb_insert(unsigned long long* list, uint32_t K, unsigned long long key,
                                 uint32_t lane) {
  const unsigned long long e = lane < K ? list[lane] : 0ull;
  const uint32_t pos = (uint32_t)__popcll(__ballot(lane < K && e > key));
  if (pos >= K) return;
  const unsigned long long up = __shfl_up(e, 1);
  if (lane < K && lane >= pos) list[lane] = lane == pos ? key : up;
}

// the first word k >= from set in both sa and sb (nkw words of bits), FS_NONE without one; the
// same in every lane
__device__ inline uint32_t nb_next(const unsigned long long* sa, const unsigned long long* sb,
                                   uint32_t nkw, uint32_t from) {
  for (uint32_t kw = from / 64; kw < nkw; ++kw) {
    unsigned long long m = wave_first(sa[kw] & sb[kw]);
    if (kw == from / 64) m &= ~0ull << (from % 64);
    if (m) return kw * 64 + (uint32_t)__builtin_ctzll(m);
  }
  return FS_NONE;
}

// The 64 x 64 scores of row tile `ra` against column tile `cb` (the matrix's layout) in a wave,
// over the words k set in both sa and sb (nkw words of bits, wave-uniform): acc[i][j][r] is row
// 16 i + 4 (lane >> 4) + r, column 16 j + (lane & 15).
template <bool kMfma>
__device__ inline void nb_scores(const unsigned long long* ra, const unsigned long long* cb,
                                 const unsigned long long* sa, const unsigned long long* sb,
                                 const uint8_t* wb, uint32_t nkw, uint32_t lane,
                                 v4i (&acc)[kFr][kFr]) {
  const uint32_t col = lane & 15, grp = lane >> 4;
#pragma unroll
  for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
    for (uint32_t j = 0; j < kFr; ++j) acc[i][j] = v4i{0, 0, 0, 0};
  if constexpr (kMfma) {
    // byte e of lane group g is script word 64 k + 16 g + e on either side
    for (uint32_t k = nb_next(sa, sb, nkw, 0); k != FS_NONE; k = nb_next(sa, sb, nkw, k + 1)) {
      const v4i wv = *reinterpret_cast<const v4i*>(wb + (size_t)k * 64 + grp * 16);
      v4i af[kFr], bf[kFr];
#pragma unroll
      for (uint32_t i = 0; i < kFr; ++i) {
        af[i] = spread16((uint32_t)(ra[(size_t)k * kTile + 16 * i + col] >> (16 * grp)) & 0xFFFFu);
        const v4i b = spread16((uint32_t)(cb[(size_t)k * kTile + 16 * i + col] >> (16 * grp)) &
                               0xFFFFu);
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d)
          bf[i][d] = (int)(((uint32_t)b[d] * 255u) & (uint32_t)wv[d]);
      }
#pragma unroll
      for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
        for (uint32_t j = 0; j < kFr; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  } else {
    for (uint32_t k = nb_next(sa, sb, nkw, 0); k != FS_NONE; k = nb_next(sa, sb, nkw, k + 1)) {
      const uint8_t* wp = wb + (size_t)k * 64;
      unsigned long long c[kFr];
#pragma unroll
      for (uint32_t j = 0; j < kFr; ++j) c[j] = cb[(size_t)k * kTile + 16 * j + col];
#pragma unroll
      for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
          const unsigned long long x = ra[(size_t)k * kTile + 16 * i + 4 * grp + r];
#pragma unroll
          for (uint32_t j = 0; j < kFr; ++j) {
            unsigned long long both = x & c[j];
            while (both) {
              acc[i][j][r] += (int)wp[(uint32_t)__builtin_ctzll(both)];
              both &= both - 1;
            }
          }
        }
    }
  }
}

// blockIdx.x = stripe (row tile), blockIdx.y = share of the column tiles.  Dynamic LDS: the
// lists of the four waves, [kWaves][64][K] keys
template <bool kMfma>
__global__ __launch_bounds__(kProd) void k_nb_product(NbArgs a) {
  extern __shared__ __align__(16) unsigned long long s_lists[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t col = lane & 15, grp = lane >> 4;
  const uint32_t ti = blockIdx.x, K = a.K;
  const uint32_t per = (a.n_tiles + a.S - 1) / a.S;
  const uint32_t t0 = blockIdx.y * per;                  // (at or past n_tiles: an empty share)
  const uint32_t t1 = a.n_tiles - (t0 < a.n_tiles ? t0 : a.n_tiles) < per ? a.n_tiles : t0 + per;
  unsigned long long* list = s_lists + (size_t)wave * kTile * K;   // the wave's own: no barrier
  for (uint32_t v = lane; v < kTile * K; v += 64) list[v] = 0ull;
  uint32_t own_a[kFr][4], cnt[kFr][4];
#pragma unroll
  for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      own_a[i][r] = a.own[(size_t)ti * kTile + 16 * i + 4 * grp + r];
      cnt[i][r] = 0;
    }
  const unsigned long long* ra = a.cov + (size_t)ti * a.nk * kTile;
  for (uint32_t tj = t0 + wave; tj < t1; tj += kWaves) {
    v4i acc[kFr][kFr];
    nb_scores<kMfma>(ra, a.cov + (size_t)tj * a.nk * kTile, a.some + (size_t)ti * a.nkw,
                     a.some + (size_t)tj * a.nkw, a.wb, a.nkw, lane, acc);
    const bool diag = tj == ti;
    uint32_t own_b[kFr];
#pragma unroll
    for (uint32_t j = 0; j < kFr; ++j) own_b[j] = a.own[(size_t)tj * kTile + 16 * j + col];
#pragma unroll
    for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
      for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t row = 16 * i + 4 * grp + r;
        // the ppm of the row's K-th key, 0 while the list has room: floor(x / den) >= t is
        // x >= t * den
        const uint64_t kth = list[row * K + K - 1] >> 32;
#pragma unroll
        for (uint32_t j = 0; j < kFr; ++j) {
          const uint32_t s = (uint32_t)acc[i][j][r];
          const uint32_t den = own_a[i][r] + own_b[j] - s;
          const uint64_t x = (uint64_t)s * kMillion;
          const bool is = s >= a.min_score && x >= (uint64_t)a.min_ppm * den &&
                          !(diag && row == 16 * j + col);
          cnt[i][r] += is;
          const bool pass = is && x >= kth * den;
          uint64_t m = __ballot(pass);
          if (!m) continue;
          unsigned long long key = 0ull;                 // (den >= own_a >= s >= 1 where is)
          if (pass) key = ((x / den) << 32) | (0xFFFFFFFFu - (tj * kTile + 16 * j + col));
          do {
            const uint32_t l = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            nb_insert(list + (16 * i + 4 * (l >> 4) + r) * K, K, __shfl(key, (int)l), lane);
          } while (m);
        }
      }
  }
  const uint32_t p = blockIdx.y * kWaves + wave;
  for (uint32_t v = lane; v < kTile * K; v += 64)
    a.part[(((size_t)ti * kTile + v / K) * a.P + p) * K + v % K] = list[v];
#pragma unroll
  for (uint32_t i = 0; i < kFr; ++i)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t c = seg_sum(cnt[i][r], 16u);
      if (col == 0) a.pcand[((size_t)ti * kTile + 16 * i + 4 * grp + r) * a.P + p] = c;
    }
}

// a wave per row: slot `lane` of the merged list in lane's register
__global__ __launch_bounds__(kRunBlock) void k_nb_merge(NbArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const size_t row = (size_t)blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (row >= (size_t)a.n_tiles * kTile) return;
  const uint32_t K = a.K;
  unsigned long long mine = 0ull;
  uint32_t c = 0;
  for (uint32_t p = 0; p < a.P; ++p) {
    const unsigned long long* src = a.part + (row * a.P + p) * K;
    for (uint32_t s = 0; s < K; ++s) {
      const unsigned long long key = src[s];             // (the same in every lane)
      if (!key) break;
      const uint32_t pos = (uint32_t)__popcll(__ballot(lane < K && mine > key));
      if (pos >= K) break;                               // sorted: the rest is smaller still
      const unsigned long long up = __shfl_up(mine, 1);
      if (lane < K && lane >= pos) mine = lane == pos ? key : up;
    }
    c += a.pcand[row * a.P + p];
  }
  if (lane < K) a.lists[row * K + lane] = mine;
  const uint32_t n = (uint32_t)__popcll(__ballot(lane < K && mine != 0ull));
  if (lane == 0) {
    a.listed[row] = n;
    a.cand[row] = c;
  }
}

__device__ inline uint32_t nb_partner(unsigned long long key) {
  return 0xFFFFFFFFu - (uint32_t)key;
}

// a lane per list slot
__global__ __launch_bounds__(kRunBlock) void k_nb_back(NbArgs a) {
  const uint64_t at = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (at >= (uint64_t)a.n_tiles * kTile * a.K) return;
  const uint32_t row = (uint32_t)(at / a.K);
  const unsigned long long key = a.lists[at];
  uint32_t found = FS_NONE;
  if (key) {
    const uint32_t b = nb_partner(key);                  // (an active number: below n_active)
    const unsigned long long* theirs = a.lists + (size_t)b * a.K;
    for (uint32_t s = 0; s < a.K && theirs[s]; ++s)
      if (nb_partner(theirs[s]) == row) {
        found = s + 1;
        break;
      }
    atomicAdd(&a.listed_by[b], 1u);
    if (found != FS_NONE) atomicAdd(&a.mutual[row], 1u);
  }
  a.back[at] = found;
}

// one lane per work (flag null: no active work)
__global__ __launch_bounds__(kRunBlock) void k_nb_works(NbArgs a, const uint32_t* flag) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.n_works) return;
  uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = make_uint4(0u, 0u, FS_NONE, 0u);
  if (flag && flag[w]) {
    const uint32_t ai = a.act[w];
    lo = make_uint4(a.covered[ai], a.own[ai], a.cand[ai], a.listed[ai]);
    hi.x = a.listed_by[ai];
    hi.y = a.mutual[ai];
    if (lo.w) {
      const unsigned long long key = a.lists[(size_t)ai * a.K];
      hi.z = a.work_of[nb_partner(key)];
      hi.w = (uint32_t)(key >> 32);
    }
  }
  uint4* o = reinterpret_cast<uint4*>(a.works + w);
  o[0] = lo;
  o[1] = hi;
}

// a lane per list slot: the head of its listed pair
__global__ __launch_bounds__(kRunBlock) void k_nb_place(NbArgs a) {
  const uint64_t at = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (at >= (uint64_t)a.n_tiles * kTile * a.K) return;
  const uint32_t row = (uint32_t)(at / a.K), s = (uint32_t)(at % a.K);
  if (s >= a.listed[row]) return;
  const unsigned long long key = a.lists[at];
  uint4* o = reinterpret_cast<uint4*>(a.out + a.off[row] + s);
  o[0] = make_uint4(a.work_of[row], a.work_of[nb_partner(key)], s + 1, a.back[at]);
  o[1] = make_uint4((uint32_t)(key >> 32), 0u, 0u, 0u);
  o[2] = make_uint4(0u, 0u, 0u, 0u);
}

// One lane per listed pair: the AND of the two rows walked a 64-bit word at a time.
__global__ __launch_bounds__(kRunBlock) void k_nb_detail(NbArgs a, uint64_t n_listed) {
  const uint64_t p = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (p >= n_listed) return;
  uint4* o = reinterpret_cast<uint4*>(a.out + p);
  const uint4 head = o[0];
  const uint32_t ia = a.act[head.x], ib = a.act[head.y];
  const unsigned long long* ra = a.cov + (size_t)(ia / kTile) * a.nk * kTile + ia % kTile;
  const unsigned long long* rb = a.cov + (size_t)(ib / kTile) * a.nk * kTile + ib % kTile;
  uint32_t shared = 0, score = 0, rare = 0, rare_w = 0;
  for (uint32_t k = 0; k < a.nk; ++k) {
    unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    shared += (uint32_t)__popcll(x);
    while (x) {
      const uint32_t at = k * 64 + (uint32_t)__builtin_ctzll(x);
      const uint32_t w = a.wb[at];
      score += w;
      if (w > rare_w) {                                  // the first among equals
        rare_w = w;
        rare = at;
      }
      x &= x - 1;
    }
  }
  // the run around `rare` (a listed pair shares a word: score >= 1): down to the clear bit
  // below it, up to the clear bit above it
  uint32_t first = 0, end = a.nk * 64;                   // (bits at n_script and above are clear)
  for (uint32_t k = rare / 64, b = rare % 64;; --k, b = 63) {
    const unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    const unsigned long long clear = ~x & (b == 63 ? ~0ull : (1ull << (b + 1)) - 1);
    if (clear) {
      first = k * 64 + 64 - (uint32_t)__builtin_clzll(clear);
      break;
    }
    if (k == 0) break;
  }
  for (uint32_t k = rare / 64, b = rare % 64; k < a.nk; ++k, b = 0) {
    const unsigned long long x = ra[(size_t)k * kTile] & rb[(size_t)k * kTile];
    const unsigned long long clear = ~x & (~0ull << b);
    if (clear) {
      end = k * 64 + (uint32_t)__builtin_ctzll(clear);
      break;
    }
  }
  const uint32_t ppm = o[1].x;
  o[1] = make_uint4(ppm, score, shared, rare);
  o[2] = make_uint4(a.depth[rare], rare_w, first, end - first);
}

// coverage, weights, product, place, detail, their total
thread_local double t_ms[6];

// one call: count() through the works and words tables and the number of listed pairs, then
// write()
struct NbJob {
  CoverJob cj;
  DBuf<uint32_t> depth, own, pcand, back, rowtab;
  DBuf<uint8_t> wb;
  DBuf<unsigned long long> some, part, lists, off, total;
  Clock<8> clk;
  NbArgs a{};
  uint64_t n_listed = 0;

  // d_works and d_words written, n_listed set (all on `s`, finished on return)
  int count(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
            uint32_t min_words, uint32_t max_gap, uint32_t weight, uint32_t top,
            uint32_t min_score, uint32_t min_similarity, fs_neighbour_work* d_works,
            fs_neighbour_word* d_words, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    const uint32_t mfma = env_u32("FS_NEIGHBOURS_MFMA", kMfmaDefault, 1u);
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.K = top;
    a.flat = weight == FS_NEIGHBOURS_FLAT;
    a.min_score = min_score;
    a.min_ppm = min_similarity * 10000u;
    a.works = d_works;
    a.words = d_words;
    const dim3 work_grid(blocks_of(n_works, kRunBlock)), blk(kRunBlock);
    if (n) FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) {
      if (n_script)
        FS_HIP(hipMemsetAsync(d_words, 0, (size_t)n_script * sizeof(fs_neighbour_word), s));
      if (n_works) hipLaunchKernelGGL(k_nb_works, work_grid, blk, 0, s, a, nullptr);
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));
      return FS_OK;
    }
    // few stripes: the column tiles are shared out until there are kSplitBlocks workgroups, at
    // least kSplitTiles tiles each (FS_NEIGHBOURS_SPLIT: that many shares, for the tests)
    uint32_t split = env_u32("FS_NEIGHBOURS_SPLIT", 0u, 65535u);
    if (!split && a.n_tiles < kSplitBlocks) {
      const uint32_t room = (kSplitBlocks + a.n_tiles - 1) / a.n_tiles;
      const uint32_t most = (a.n_tiles + kSplitTiles - 1) / kSplitTiles;
      split = room < most ? room : most;
    }
    if (split > a.n_tiles) split = a.n_tiles;
    a.S = split ? split : 1u;
    a.P = a.S * kWaves;
    a.nkw = (a.nk + 63) / 64;
    const size_t rows = (size_t)a.n_tiles * kTile, kw = (size_t)a.nk * 64;
    const size_t n_some = (size_t)a.n_tiles * a.nkw;
    const uint64_t bytes = (uint64_t)rows * a.nk * 8 + (uint64_t)rows * a.P * top * 8 +
                           (uint64_t)rows * a.P * 4 + (uint64_t)rows * top * 12 + (uint64_t)kw * 5 + (uint64_t)n_some * 8;
    if (bytes > FS_NEIGHBOURS_MAX_BYTES) {
      fs_set_error("%u works with a passage over %u script words, lists of %u in %u shares: a "
                   "coverage matrix, lists and weights of %llu bytes, more than %u", a.n_active,
                   n_script, top, a.S, (unsigned long long)bytes, FS_NEIGHBOURS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(cj.reserve(a, s));
    FS_TRY(depth.reserve(kw));
    FS_TRY(wb.reserve(kw));
    FS_TRY(some.reserve(n_some));
    FS_TRY(own.reserve(rows));
    FS_TRY(part.reserve(rows * a.P * top));
    FS_TRY(pcand.reserve(rows * a.P));
    FS_TRY(lists.reserve(rows * top));
    FS_TRY(back.reserve(rows * top));
    FS_TRY(rowtab.reserve(rows * 4));                    // cand, listed, listed_by, mutual
    FS_TRY(off.reserve(rows));
    FS_TRY(total.reserve(1));
    FS_HIP(hipMemsetAsync(depth.p, 0, kw * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(some.p, 0, n_some * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(rowtab.p, 0, rows * 4 * sizeof(uint32_t), s));
    a.depth = depth.p;
    a.wb = wb.p;
    a.some = some.p;
    a.own = own.p;
    a.part = part.p;
    a.pcand = pcand.p;
    a.lists = lists.p;
    a.back = back.p;
    a.cand = rowtab.p;
    a.listed = rowtab.p + rows;
    a.listed_by = rowtab.p + 2 * rows;
    a.mutual = rowtab.p + 3 * rows;
    a.off = off.p;
    a.total = total.p;
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    FS_TRY(clk.mark(1, s));
    uint32_t gy = 1024u / a.nk;
    const uint32_t most = blocks_of(a.n_tiles, kRunBlock / 64);
    gy = gy < 1u ? 1u : gy > most ? most : gy;
    hipLaunchKernelGGL(k_nb_depth, dim3(a.nk, gy), blk, 0, s, a);
    hipLaunchKernelGGL(k_nb_weight, dim3(blocks_of(kw, kRunBlock)), blk, 0, s, a);
    hipLaunchKernelGGL(k_nb_own, dim3(a.n_tiles), dim3(kTile), 0, s, a);
    FS_TRY(clk.mark(2, s));
    const size_t lds = (size_t)kWaves * kTile * top * sizeof(unsigned long long);
    if (mfma)
      hipLaunchKernelGGL(k_nb_product<true>, dim3(a.n_tiles, a.S), dim3(kProd), lds, s, a);
    else
      hipLaunchKernelGGL(k_nb_product<false>, dim3(a.n_tiles, a.S), dim3(kProd), lds, s, a);
    hipLaunchKernelGGL(k_nb_merge, dim3(blocks_of(rows, kRunBlock / 64)), blk, 0, s, a);
    FS_TRY(clk.mark(3, s));
    hipLaunchKernelGGL(k_nb_back, dim3(blocks_of(rows * top, kRunBlock)), blk, 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<unsigned long long>, dim3(1), dim3(kScanBlock), 0, s,
                       a.listed, (uint64_t)rows, off.p, total.p);
    hipLaunchKernelGGL(k_nb_works, work_grid, blk, 0, s, a, cj.flag.p);
    FS_TRY(clk.mark(4, s));
    FS_HIP(hipGetLastError());
    unsigned long long tot = 0;
    FS_HIP(hipMemcpyAsync(&tot, total.p, sizeof tot, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    n_listed = tot;
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    t_ms[2] = clk.elapsed(2, 3);
    t_ms[3] = clk.elapsed(3, 4);
    t_ms[5] = t_ms[0] + t_ms[1] + t_ms[2] + t_ms[3];
    return FS_OK;
  }

  // the n_listed pairs into d_out (finished on return)
  int write(fs_neighbour* d_out, hipStream_t s) {
    if (!n_listed) return FS_OK;
    a.out = d_out;
    const size_t slots = (size_t)a.n_tiles * kTile * a.K;
    FS_TRY(clk.mark(5, s));
    hipLaunchKernelGGL(k_nb_place, dim3(blocks_of(slots, kRunBlock)), dim3(kRunBlock), 0, s, a);
    FS_TRY(clk.mark(6, s));
    hipLaunchKernelGGL(k_nb_detail, dim3(blocks_of(n_listed, kRunBlock)), dim3(kRunBlock), 0, s, a,
                       (uint64_t)n_listed);
    FS_TRY(clk.mark(7, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[3] += clk.elapsed(5, 6);
    t_ms[4] = clk.elapsed(6, 7);
    t_ms[5] += clk.elapsed(5, 7);
    return FS_OK;
  }
};

// the rules both entry points share
int nb_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
             uint32_t weight, uint32_t top, uint32_t min_score, uint32_t min_similarity,
             const void* works, const void* words, const void* listed, uint64_t cap,
             uint64_t* n_listed) {
  if (!n_listed || (n_works && !works) || (n_script && !words) || (cap && !listed)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_score == 0) {
    fs_set_error("min_words and min_score must be at least 1");
    return FS_E_INVALID;
  }
  if (weight != FS_NEIGHBOURS_RARITY && weight != FS_NEIGHBOURS_FLAT) {
    fs_set_error("weight %u: FS_NEIGHBOURS_RARITY or FS_NEIGHBOURS_FLAT", weight);
    return FS_E_INVALID;
  }
  if (top == 0 || top > kMaxTop) {
    fs_set_error("top %u: from 1 to %u", top, kMaxTop);
    return FS_E_INVALID;
  }
  if (min_similarity > 100) {
    fs_set_error("min_similarity %u: a whole percentage, 0 to 100", min_similarity);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("neighbours", n_rows, n_script));
  *n_listed = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_neighbours(int device, const uint32_t* work, const uint32_t* fan_ix,
                             const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                             uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                             uint32_t weight, uint32_t top, uint32_t min_score,
                             uint32_t min_similarity, fs_neighbour_work* works,
                             fs_neighbour_word* words, fs_neighbour* listed, uint64_t cap,
                             uint64_t* n_listed) {
  FS_TRY(nb_check(n_rows, n_works, n_script, min_words, weight, top, min_score, min_similarity,
                  works, words, listed, cap, n_listed));
  if (!n_rows) {
    const fs_neighbour_work none{0u, 0u, 0u, 0u, 0u, 0u, FS_NONE, 0u};
    for (uint32_t w = 0; w < n_works; ++w) works[w] = none;
    for (uint32_t o = 0; o < n_script; ++o) words[o] = fs_neighbour_word{0u, 0u};
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_neighbour_work> d_works;
  DBuf<fs_neighbour_word> d_words;
  DBuf<fs_neighbour> d_out;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_works.reserve(n_works));
  FS_TRY(d_words.reserve(n_script));
  NbJob job;
  FS_TRY(job.count(rows.p, n, n_works, n_script, min_words, max_gap, weight, top, min_score,
                   min_similarity, d_works.p, d_words.p, nullptr));
  if (n_works) FS_TRY(copy_out(works, d_works, n_works));
  if (n_script) FS_TRY(copy_out(words, d_words, n_script));
  *n_listed = job.n_listed;
  if (job.n_listed > cap) return FS_E_CAPACITY;
  if (job.n_listed) {
    FS_TRY(d_out.reserve(job.n_listed));
    FS_TRY(job.write(d_out.p, nullptr));
    FS_TRY(copy_out(listed, d_out, job.n_listed));
  }
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_neighbours_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                  uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                                  uint32_t weight, uint32_t top, uint32_t min_score,
                                  uint32_t min_similarity, fs_neighbour_work* d_works,
                                  fs_neighbour_word* d_words, fs_neighbour* d_listed,
                                  uint64_t cap, uint64_t* n_listed) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: neighbours take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(nb_check(n_rows, n_works, (uint32_t)ix->n_script, min_words, weight, top, min_score,
                  min_similarity, d_works, d_words, d_listed, cap, n_listed));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_works & 15) ||
      ((uintptr_t)d_words & 15) || ((uintptr_t)d_listed & 15)) {
    fs_set_error("d_rows, d_works, d_words and d_listed must be 16-byte aligned device pointers");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  NbJob job;
  FS_TRY(job.count(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                   weight, top, min_score, min_similarity, d_works, d_words, ix->stream));
  *n_listed = job.n_listed;
  if (job.n_listed > cap) return FS_E_CAPACITY;
  return job.write(d_listed, ix->stream);
}

extern "C" int fs_neighbours_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
