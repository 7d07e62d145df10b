// fs_contrast.hip -- `ao3.py contrast`: what one set of fan works quotes more than another, a
// permutation test of every unit at once with the max-statistic correction (fs_contrast,
// fs_contrast_rows in include/fandom_search.h).  Permutation r relabels the pool: its side A is
// the NA pool works smallest in (key(r, w), w), a pure function of (seed, r, w).  The recount of
// every unit under every relabelling is one product, counts = M x L^T, of the unit x work
// incidence bit matrix M of fs_incidence.h and the labels L, a bit per (permutation, active
// work) in the same layout.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   k_con_sides      a lane per work: a side byte above 2, NA and N
//   incidence        IncJob of fs_incidence.h: M and the active numbering, without works(u)
//   k_con_select     a workgroup per row of L.  A permutation: the NA-th smallest key by a radix
//                    select over 12 + 12 + 8 bits, a histogram in LDS per pass and the hash made
//                    again in each (no N x P keys are stored); the works at the boundary key in
//                    ascending work number, each wave counting those of a contiguous quarter of
//                    the works and the wave that holds the last one taken finding it; then the
//                    labels of the active works, one ballot per 64 active numbers, and their
//                    number.  Rows P and P + 1: the observed side A and the pool
//   k_con_product    the hot path: a workgroup per (tile of 64 units, tile of 64 rows of L), the
//                    64 x 64 AND/popcounts of tile_counts, written with the rows of L adjacent
//   k_con_sweep      a wave per unit: a, b, D, den, X, GE; a family unit raises MX[r] by a
//                    64-bit atomic max, read first and left out where it cannot win
//   k_con_adjust     MX in LDS; a wave per family unit: ADJ_GE, and an atomic min into
//                    MAX_UNIT[r] where the unit attains MX[r]
//   k_con_perms      a lane per permutation: its fs_contrast_perm
//   k_con_none       no active work: every count is 0
#include "fs_incidence.h"

#include <math.h>
#include <string.h>

namespace {

constexpr uint32_t kSel = 256;                // threads of k_con_select
constexpr uint32_t kBins = 4096;              // bins of its first two passes; 256 in the third
constexpr uint32_t kAdjUnits = 64;            // units a workgroup of k_con_adjust takes
constexpr uint32_t kMaxPerms = FS_CONTRAST_MAX_PERMUTATIONS;

struct ConArgs : IncArgs {
  uint32_t P, R, Rp;            // permutations; rows of L: P + 2; padded to a multiple of 64
  uint32_t NA, N;               // works of side A and of the pool
  uint32_t key_bits, min_quoting, precheck;
  uint64_t term;                // seed * 0x9E3779B97F4A7C15
  const uint8_t* side;          // [r.n_works]
  unsigned long long* lab;      // L: [Rp / 64][m.nk][64]
  uint32_t* counts;             // [m.n_tiles * 64][Rp]
  uint32_t* a_act;              // [P] active works drawn into side A
  unsigned long long* mx;       // [P] MX_r
  uint32_t* mu;                 // [P] MAX_UNIT_r
  fs_contrast_unit* units;
  fs_contrast_perm* perms;
};

// the exact floor of the square root: the double's is off by one where x has more than 53 bits
__host__ __device__ inline uint64_t con_isqrt(uint64_t x) {
  uint64_t s = (uint64_t)sqrt((double)x);
  if (s > 0xFFFFFFFFull) s = 0xFFFFFFFFull;
  while (s * s > x) --s;
  while (s < 0xFFFFFFFFull && (s + 1) * (s + 1) <= x) ++s;
  return s;
}

__device__ inline uint32_t con_key(const ConArgs& a, uint32_t r, uint32_t w) {
  return a.key_bits ? fs_work_hash(a.term, r, w) >> (32u - a.key_bits) : 0u;
}

__device__ inline uint64_t con_abs(int64_t d) {
  return d < 0 ? (uint64_t)-d : (uint64_t)d;
}

// tally: [0] a byte above 2, [1] NA, [2] N
__global__ __launch_bounds__(kRunBlock) void k_con_sides(const uint8_t* side, uint32_t n_works,
                                                         uint32_t* tally) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t s = w < n_works ? side[w] : 0u;
  const uint64_t bad = __ballot(s > 2), in_a = __ballot(s == 1), in_b = __ballot(s == 2);
  if (threadIdx.x & 63) return;
  if (bad) atomicOr(&tally[0], 1u);
  if (in_a) atomicAdd(&tally[1], (uint32_t)__popcll(in_a));
  if (in_a | in_b) atomicAdd(&tally[2], (uint32_t)__popcll(in_a | in_b));
}

// blockIdx.x = row of L
__global__ __launch_bounds__(kSel) void k_con_select(ConArgs a) {
  __shared__ uint32_t s_hist[kBins];
  __shared__ uint32_t s_w[kSel / 64];
  __shared__ uint32_t s_pick[2];
  const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t nw = a.r.n_works;
  const bool perm = r < a.P && a.NA;              // (NA = 0: nobody is drawn)
  uint32_t K = 0, wstar = 0;                      // side A: key < K, or key == K and w <= wstar
  if (perm) {
    // the NA-th smallest key: `rank` among the pool works whose key has `prefix` under `pmask`
    uint32_t prefix = 0, pmask = 0, rank = a.NA;
    for (uint32_t pass = 0; pass < 3; ++pass) {
      const uint32_t shift = pass == 0 ? 20u : pass == 1 ? 8u : 0u;
      const uint32_t nb = pass < 2 ? kBins : 256u, per = nb / kSel;
      for (uint32_t i = tid; i < nb; i += kSel) s_hist[i] = 0;
      __syncthreads();
      for (uint32_t w = tid; w < nw; w += kSel) {
        if (!a.side[w]) continue;
        const uint32_t k = con_key(a, r, w);
        if ((k & pmask) == prefix) atomicAdd(&s_hist[(k >> shift) & (nb - 1)], 1u);
      }
      __syncthreads();
      uint32_t mine = 0, total;
      for (uint32_t j = 0; j < per; ++j) mine += s_hist[tid * per + j];
      const uint32_t pre = block_scan<kSel>(mine, s_w, &total);
      if (pre < rank && rank <= pre + mine) {     // one thread: 1 <= rank <= total
        uint32_t c = pre;
        for (uint32_t j = 0; j < per; ++j) {
          const uint32_t h = s_hist[tid * per + j];
          if (rank <= c + h) {
            s_pick[0] = tid * per + j;
            s_pick[1] = rank - c;
            break;
          }
          c += h;
        }
      }
      __syncthreads();
      prefix |= s_pick[0] << shift;
      pmask |= (nb - 1) << shift;
      rank = s_pick[1];
      __syncthreads();                            // s_pick and s_hist are written again
    }
    K = prefix;
    // `rank` of the pool works with key K are drawn, in ascending work number: wave v counts
    // those of works v * seg .. (v + 1) * seg, the wave that holds the last one finds it
    const uint32_t seg = ((nw + kSel / 64 - 1) / (kSel / 64) + 63) / 64 * 64;
    const uint32_t w0 = wave * seg < nw ? wave * seg : nw;
    const uint32_t w1 = nw - w0 < seg ? nw : w0 + seg;
    uint32_t ties = 0;
    for (uint32_t b = w0; b < w1; b += 64) {
      const uint32_t w = b + lane;
      const bool eq = w < w1 && a.side[w] && con_key(a, r, w) == K;
      ties += (uint32_t)__popcll(__ballot(eq));
    }
    if (lane == 0) s_w[wave] = ties;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t v = 0; v < wave; ++v) before += s_w[v];
    if (before < rank && rank <= before + ties) {   // one wave
      uint32_t c = before;
      for (uint32_t b = w0; b < w1; b += 64) {
        const uint32_t w = b + lane;
        const bool eq = w < w1 && a.side[w] && con_key(a, r, w) == K;
        const uint64_t m = __ballot(eq);
        const uint32_t pc = (uint32_t)__popcll(m);
        if (rank <= c + pc) {
          if (eq && c + (uint32_t)__popcll(m & ((1ull << lane) - 1)) + 1 == rank) s_pick[0] = w;
          break;
        }
        c += pc;
      }
    }
    __syncthreads();
    wstar = s_pick[0];
    __syncthreads();                              // s_w is written again
  }
  // the labels of the active works: wave v the words v, v + 4, ...
  uint32_t drawn = 0;
  unsigned long long* out = a.lab + (size_t)(r / kTile) * a.m.nk * kTile + r % kTile;
  for (uint32_t k = wave; k < a.m.nk; k += kSel / 64) {
    const uint32_t w = a.r.work_of[(size_t)k * 64 + lane];       // FS_NONE: padding
    const uint32_t s = w < nw ? a.side[w] : 0u;
    bool in = false;
    if (r >= a.P) {
      in = r == a.P ? s == 1 : s != 0;
    } else if (perm && s) {
      const uint32_t key = con_key(a, r, w);
      in = key < K || (key == K && w <= wstar);
    }
    const uint64_t bits = __ballot(in);
    if (lane == 0) out[(size_t)k * kTile] = bits;
    drawn += (uint32_t)__popcll(bits);
  }
  if (r >= a.P) return;
  if (lane == 0) s_w[wave] = drawn;
  __syncthreads();
  if (tid == 0) a.a_act[r] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// blockIdx.x = tile of 64 units, blockIdx.y = tile of 64 rows of L
__global__ __launch_bounds__(kBlock) void k_con_product(ConArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  tile_counts(a.m.cov + (size_t)blockIdx.x * a.m.nk * kTile,
              a.lab + (size_t)blockIdx.y * a.m.nk * kTile, a.m.nk, s_a, s_b, s_sh);
  uint32_t* out = a.counts + (size_t)blockIdx.x * kTile * a.Rp + (size_t)blockIdx.y * kTile;
  for (uint32_t v = threadIdx.x; v < kTile * kTile; v += kBlock) {
    const uint32_t i = v / kTile, j = v % kTile;             // unit, row of L
    out[(size_t)i * a.Rp + j] = s_sh[i * kShStride + j];
  }
}

// a wave per unit
__global__ __launch_bounds__(kRunBlock) void k_con_sweep(ConArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t u = blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (u >= a.n_units) return;
  const uint32_t* row = a.counts + (size_t)u * a.Rp;
  const uint32_t au = row[a.P], t = row[a.P + 1];
  const int64_t base = (int64_t)t * a.NA;
  const int64_t D = (int64_t)au * a.N - base;
  const uint64_t absD = con_abs(D);
  const uint64_t den = con_isqrt(((uint64_t)t * (a.N - t)) << 20);
  const bool family = t >= a.min_quoting && den;             // (den = 0: every X is 0)
  uint32_t ge = 0;
  for (uint32_t r = lane; r < a.P; r += 64) {
    const uint64_t ad = con_abs((int64_t)row[r] * a.N - base);
    ge += ad >= absD;
    if (!family || !ad) continue;
    const unsigned long long x = (ad << 20) / den;
    if (x && (!a.precheck || x > a.mx[r])) atomicMax(&a.mx[r], x);
  }
  ge = wave_sum(ge);
  if (lane) return;
  fs_contrast_unit* v = a.units + u;
  v->a_works = au;
  v->b_works = t - au;
  v->ge = ge;
  v->adj_ge = FS_NONE;
  v->statistic = den ? (absD << 20) / den : 0ull;
  v->d = D;
}

// blockIdx.x = kAdjUnits units, a wave per unit in turn
__global__ __launch_bounds__(kRunBlock) void k_con_adjust(ConArgs a) {
  __shared__ unsigned long long s_mx[kMaxPerms];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t r = threadIdx.x; r < a.P; r += kRunBlock) s_mx[r] = a.mx[r];
  __syncthreads();
  const uint32_t u0 = blockIdx.x * kAdjUnits;
  const uint32_t u1 = a.n_units - u0 < kAdjUnits ? a.n_units : u0 + kAdjUnits;
  for (uint32_t u = u0 + wave; u < u1; u += kRunBlock / 64) {
    const uint32_t* row = a.counts + (size_t)u * a.Rp;
    const uint32_t t = row[a.P + 1];
    if (t < a.min_quoting) continue;
    const int64_t base = (int64_t)t * a.NA;
    const uint64_t den = con_isqrt(((uint64_t)t * (a.N - t)) << 20);
    const uint64_t X = a.units[u].statistic;
    uint32_t adj = 0;
    for (uint32_t r = lane; r < a.P; r += 64) {
      const uint64_t ad = con_abs((int64_t)row[r] * a.N - base);
      const uint64_t x = den ? (ad << 20) / den : 0ull;
      adj += s_mx[r] >= X;
      if (x == s_mx[r]) atomicMin(&a.mu[r], u);
    }
    adj = wave_sum(adj);
    if (lane == 0) a.units[u].adj_ge = adj;
  }
}

// one lane per permutation
__global__ __launch_bounds__(kRunBlock) void k_con_perms(ConArgs a) {
  const uint32_t r = blockIdx.x * kRunBlock + threadIdx.x;
  if (r >= a.P) return;
  const unsigned long long x = a.mx[r];
  reinterpret_cast<uint4*>(a.perms)[r] =
      make_uint4((uint32_t)x, (uint32_t)(x >> 32), a.a_act[r], a.mu[r]);
}

// one lane per unit, when no work is active: nobody quotes it under any labelling
__global__ __launch_bounds__(kRunBlock) void k_con_none(ConArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u >= a.n_units) return;
  uint4* p = reinterpret_cast<uint4*>(a.units + u);
  p[0] = make_uint4(0u, 0u, a.P, FS_NONE);
  p[1] = make_uint4(0u, 0u, 0u, 0u);
}

// incidence, selection, product, sweeps, their total
thread_local double t_ms[5];

struct ConJob {
  IncJob inc;
  DBuf<uint32_t> tally, counts, a_act, mu;
  DBuf<unsigned long long> lab, mx;
  Clock<5> clk;
  ConArgs a{};

  // d_units and d_perms written, and h_counts (host, [n_units][permutations]) unless null (all
  // on `s`, finished on return)
  int run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
          const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
          const uint8_t* d_side, uint32_t min_quoting, uint32_t permutations, uint64_t seed,
          uint32_t key_bits, fs_contrast_unit* d_units, fs_contrast_perm* d_perms,
          uint32_t* h_counts, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    const uint64_t max_bytes =
        env_u32("FS_CONTRAST_MAX_BYTES", FS_CONTRAST_MAX_BYTES, FS_CONTRAST_MAX_BYTES);
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.P = permutations;
    a.R = permutations + 2;
    a.Rp = (a.R + kTile - 1) / kTile * kTile;
    a.key_bits = key_bits;
    a.min_quoting = min_quoting;
    a.precheck = env_u32("FS_CONTRAST_PRECHECK", 1u, 1u);
    a.term = seed * 0x9E3779B97F4A7C15ull;
    a.side = d_side;
    a.units = d_units;
    a.perms = d_perms;
    const dim3 blk(kRunBlock);
    // the check of the sides rides in front of number(), which waits and refuses after it
    uint32_t st[3] = {0, 0, 0};
    FS_TRY(tally.reserve(3));
    FS_HIP(hipMemsetAsync(tally.p, 0, sizeof st, s));
    FS_TRY(clk.mark(0, s));
    if (n_works)
      hipLaunchKernelGGL(k_con_sides, dim3(blocks_of(n_works, kRunBlock)), blk, 0, s, d_side,
                         n_works, tally.p);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(st, tally.p, sizeof st, hipMemcpyDeviceToHost, s));
    int rc = FS_OK;
    if (n)
      rc = inc.number(d_rows, a, max_gap, s);
    else
      FS_HIP(hipStreamSynchronize(s));
    if (st[0]) {
      fs_set_error("a side byte above 2 (0 out, 1 side A, 2 side B)");
      return FS_E_INVALID;
    }
    if (rc != FS_OK) return rc;
    a.NA = st[1];
    a.N = st[2];
    const bool some = n && a.r.n_active;
    FS_TRY(a_act.reserve(a.P));
    FS_TRY(mx.reserve(a.P));
    FS_TRY(mu.reserve(a.P));
    FS_HIP(hipMemsetAsync(a_act.p, 0, (size_t)a.P * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(mx.p, 0, (size_t)a.P * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(mu.p, 0xFF, (size_t)a.P * sizeof(uint32_t), s));
    a.a_act = a_act.p;
    a.mx = mx.p;
    a.mu = mu.p;
    size_t rows = 0;
    if (some) {
      rows = (size_t)a.m.n_tiles * kTile;
      const size_t nk = a.m.nk;
      const uint64_t mat_bytes = IncJob::mat_bytes(a);
      const uint64_t lab_bytes = (uint64_t)a.Rp * nk * 8;
      const uint64_t count_bytes = (uint64_t)rows * a.Rp * 4;
      if (mat_bytes + lab_bytes + count_bytes > max_bytes) {
        fs_set_error("%u units over %u works with a passage in %u permutations: an incidence "
                     "matrix of %llu bytes, labels of %llu bytes and counts of %llu bytes are "
                     "more than %llu bytes", n_units, a.r.n_active, permutations,
                     (unsigned long long)mat_bytes, (unsigned long long)lab_bytes,
                     (unsigned long long)count_bytes, (unsigned long long)max_bytes);
        return FS_E_UNSUPPORTED;
      }
      FS_TRY(inc.reserve(a, false, s));                      // with no units: work_of alone
      FS_TRY(lab.reserve((size_t)a.Rp * nk));
      FS_TRY(counts.reserve(rows * a.Rp));
      FS_HIP(hipMemsetAsync(lab.p, 0, (size_t)a.Rp * nk * sizeof(unsigned long long), s));
      a.lab = lab.p;
      a.counts = counts.p;
      inc.incidence(d_rows, a, s);
    }
    FS_TRY(clk.mark(1, s));
    if (some) hipLaunchKernelGGL(k_con_select, dim3(a.R), dim3(kSel), 0, s, a);
    FS_TRY(clk.mark(2, s));
    if (some && n_units)
      hipLaunchKernelGGL(k_con_product, dim3(a.m.n_tiles, a.Rp / kTile), dim3(kBlock), 0, s, a);
    FS_TRY(clk.mark(3, s));
    if (some && n_units) {
      hipLaunchKernelGGL(k_con_sweep, dim3(blocks_of(n_units, kRunBlock / 64)), blk, 0, s, a);
      hipLaunchKernelGGL(k_con_adjust, dim3(blocks_of(n_units, kAdjUnits)), blk, 0, s, a);
    } else if (n_units) {
      hipLaunchKernelGGL(k_con_none, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s, a);
    }
    hipLaunchKernelGGL(k_con_perms, dim3(blocks_of(a.P, kRunBlock)), blk, 0, s, a);
    FS_TRY(clk.mark(4, s));
    FS_HIP(hipGetLastError());
    if (h_counts && n_units) {
      if (some)
        FS_HIP(hipMemcpy2DAsync(h_counts, (size_t)a.P * 4, counts.p, (size_t)a.Rp * 4,
                                (size_t)a.P * 4, n_units, hipMemcpyDeviceToHost, s));
      else
        memset(h_counts, 0, (size_t)n_units * a.P * 4);
    }
    FS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) t_ms[k] = clk.elapsed(k, k + 1);
    t_ms[4] = t_ms[0] + t_ms[1] + t_ms[2] + t_ms[3];
    return FS_OK;
  }
};

// the rules both entry points share
int con_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const void* unit_of,
              uint32_t n_units, uint32_t min_words, const void* side, uint32_t min_quoting,
              uint32_t permutations, uint32_t key_bits, const void* units, const void* perms) {
  if (!perms || (n_units && !units) || (n_works && !side) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_quoting == 0) {
    fs_set_error("min_words and min_quoting must be at least 1");
    return FS_E_INVALID;
  }
  if (permutations == 0 || permutations > FS_CONTRAST_MAX_PERMUTATIONS) {
    fs_set_error("permutations %u: from 1 to %u", permutations, FS_CONTRAST_MAX_PERMUTATIONS);
    return FS_E_INVALID;
  }
  if (key_bits > 32) {
    fs_set_error("key_bits %u: from 0 to 32", key_bits);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("contrasts", n_rows, n_script));
  if (n_works > FS_CONTRAST_MAX_WORKS) {
    fs_set_error("n_works %u: contrasts take up to %u", n_works, FS_CONTRAST_MAX_WORKS);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_contrast(int device, const uint32_t* work, const uint32_t* fan_ix,
                           const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                           uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                           uint32_t min_words, uint32_t max_gap, const uint8_t* side,
                           uint32_t min_quoting, uint32_t permutations, uint64_t seed,
                           uint32_t key_bits, fs_contrast_unit* units, fs_contrast_perm* perms,
                           uint32_t* a_counts) {
  FS_TRY(con_check(n_rows, n_works, n_script, unit_of, n_units, min_words, side, min_quoting,
                   permutations, key_bits, units, perms));
  if (n_rows && (!work || !fan_ix || !orig_ix)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_unit_of;
  DBuf<uint8_t> d_side;
  DBuf<fs_contrast_unit> d_units;
  DBuf<fs_contrast_perm> d_perms;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n && n_units ? n_script : 0, nullptr));
  FS_TRY(d_side.upload(side, n_works, nullptr));
  FS_TRY(d_units.reserve(n_units));
  FS_TRY(d_perms.reserve(permutations));
  ConJob job;
  FS_TRY(job.run(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap, d_side.p,
                 min_quoting, permutations, seed, key_bits, d_units.p, d_perms.p, a_counts,
                 nullptr));
  if (n_units) FS_TRY(copy_out(units, d_units, n_units));
  FS_TRY(copy_out(perms, d_perms, permutations));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_contrast_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                                uint32_t min_words, uint32_t max_gap, const uint8_t* d_side,
                                uint32_t min_quoting, uint32_t permutations, uint64_t seed,
                                uint32_t key_bits, fs_contrast_unit* d_units,
                                fs_contrast_perm* d_perms) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: contrasts take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(con_check(n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, d_side,
                   min_quoting, permutations, key_bits, d_units, d_perms));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 15) || ((uintptr_t)d_perms & 15)) {
    fs_set_error("d_rows, d_units and d_perms must be 16-byte aligned device pointers, "
                 "d_unit_of 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  ConJob job;
  return job.run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                 min_words, max_gap, d_side, min_quoting, permutations, seed, key_bits, d_units,
                 d_perms, nullptr, ix->stream);
}

extern "C" int fs_contrast_times(double* ms) {
  return times_out(ms, t_ms, 5);
}

extern "C" uint64_t fs_contrast_isqrt(uint64_t x) {
  return con_isqrt(x);
}
