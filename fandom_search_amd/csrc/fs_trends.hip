// fs_trends.hip -- `ao3.py trends`: which units the later (or the earlier) fan works quote, a
// test of every unit at once against random re-datings of the same works, with the max-statistic
// correction of fs_contrast.hip (fs_trends, fs_trends_rows in include/fandom_search.h).  A work
// of the pool has a period offset x(w) of at most 1023; re-dating r gives every pool work the
// offset of a pool work drawn uniformly, with replacement, a pure function of (seed, r, w).  The
// sum of the offsets over the works quoting a unit, under every re-dating, is one product,
// s = M x X^T, of the unit x work incidence bit matrix M of fs_incidence.h and the offsets, ten
// bits each, held as two planes of signed bytes: x & 127 and x >> 7.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   k_trd_when       a lane per work: an offset above 1023 that is not 0xFFFF, the pool flags
//   k_pairs_scan     the pool positions and N
//   k_trd_pool       a lane per work: the offsets of the pool in pool order
//   incidence        IncJob of fs_incidence.h: M and the active numbering, without works(u)
//   k_trd_pbits      the pool as a row of bits over the active works: t(u) is an AND and a popcount
//   k_trd_labels     a lane per (row, work): the hash, the gather, X_r by a workgroup reduction
//                    and one atomic add, and for an active work the two bytes.  Row P: the
//                    observed offsets, so X_P = X
//   k_trd_product    the hot path: v_mfma_i32_16x16x64_i8 with the fragment maps at the head of
//                    fs_intervals.hip.  A workgroup takes a tile of 64 units and 128 rows, each of
//                    its four waves 64 units x 32 rows: per 64-bit word k of M four B fragments
//                    (16 units each), expanded once from bits to 0/1 bytes, against two A
//                    fragments of either plane, sixteen MFMAs an expansion and as many
//                    accumulators as k_int_product holds (with four A fragments of either plane
//                    a wave is alone on its SIMD and the product takes 1.8 times as long);
//                    s = lo + 128 hi (lo < 2^27, hi < 2^23).  With few tiles the words k are
//                    shared among workgroups that add into the sums
//   k_trd_plain      FS_TRENDS_MFMA=0: a lane per (unit, row) walks the set bits of the unit's row
//   k_trd_sweep      a wave per unit: t, the smallest and largest offset, D, den, Z, GE; a family
//                    unit raises MX[r] by a 64-bit atomic max, read first and left out where it
//                    cannot win
//   k_trd_adjust     MX in LDS; a wave per family unit: ADJ_GE, and an atomic min into
//                    MAX_UNIT[r] where the unit attains MX[r]
//   k_trd_perms      a lane per re-dating: its fs_trends_perm
//   k_trd_none       no active work: every sum is 0
#include "fs_incidence.h"
#include "fs_hash.h"

#include <math.h>
#include <string.h>

namespace {

constexpr uint32_t kProd = 256;               // threads of k_trd_product: four waves
constexpr uint32_t kUT = 4;                   // B fragments (16 units) a wave holds: a tile of M
constexpr uint32_t kRT = 2;                   // A fragments (16 rows) of either plane against them
constexpr uint32_t kAdjUnits = 64;            // units a workgroup of k_trd_adjust takes
constexpr uint32_t kMaxPerms = FS_TRENDS_MAX_PERMUTATIONS;
constexpr uint32_t kOut = 0xFFFFu;            // `when` of a work outside the pool
constexpr uint32_t kMfmaDefault = 1u;         // FS_TRENDS_MFMA unset: the faster in trends_bench.py

typedef int v4i __attribute__((ext_vector_type(4)));

struct TrdArgs : IncArgs {
  uint32_t P, R, Rp;            // re-datings; rows of a plane: P + 1; padded to a multiple of 16
  uint32_t Wp;                  // bytes of a row of a plane: m.nk * 64
  uint32_t N;                   // works of the pool
  uint32_t min_quoting;
  uint32_t ksplit;              // workgroups that share the words k of a product tile
  uint64_t term;                // seed * 0x9E3779B97F4A7C15
  const uint16_t* when;         // [r.n_works]
  const uint32_t* flag;         // [r.n_works] 1: active (null: no plane is written)
  const uint32_t* pos;          // [r.n_works] pool works in front of w
  uint16_t* pool_x;             // [N] x(pool[v])
  unsigned long long* pbits;    // [m.nk] the pool over the active numbers
  uint8_t* lo;                  // [Rp][Wp] x & 127
  uint8_t* hi;                  // [Rp][Wp] x >> 7
  uint32_t* sums;               // [m.n_tiles * 64][Rp]
  uint32_t* xr;                 // [R] X_r; xr[P] = X
  unsigned long long* mx;       // [P] MX_r
  uint32_t* mu;                 // [P] MAX_UNIT_r
  fs_trends_unit* units;
  fs_trends_perm* perms;
};

// the exact floor of the square root, as fs_contrast_isqrt computes it
__device__ inline uint64_t trd_isqrt(uint64_t x) {
  uint64_t s = (uint64_t)sqrt((double)x);
  if (s > 0xFFFFFFFFull) s = 0xFFFFFFFFull;
  while (s * s > x) --s;
  while (s < 0xFFFFFFFFull && (s + 1) * (s + 1) <= x) ++s;
  return s;
}

__device__ inline uint64_t trd_abs(int64_t d) {
  return d < 0 ? (uint64_t)-d : (uint64_t)d;
}

// a lane per work.  bad: an offset above 1023 that is not 0xFFFF
__global__ __launch_bounds__(kRunBlock) void k_trd_when(const uint16_t* when, uint32_t n_works,
                                                        uint32_t* inpool, uint32_t* bad) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t x = w < n_works ? when[w] : kOut;
  if (w < n_works) inpool[w] = x != kOut;
  if (__ballot(x != kOut && x >= FS_TRENDS_MAX_SPAN) && (threadIdx.x & 63) == 0)
    atomicOr(bad, 1u);
}

// a lane per work
__global__ __launch_bounds__(kRunBlock) void k_trd_pool(TrdArgs a) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.r.n_works) return;
  const uint16_t x = a.when[w];
  if (x != kOut && a.pos[w] < a.N) a.pool_x[a.pos[w]] = x;
}

// a lane per active number, the padding included
__global__ __launch_bounds__(kRunBlock) void k_trd_pbits(TrdArgs a) {
  const uint32_t ai = blockIdx.x * kRunBlock + threadIdx.x;
  if (ai >= a.Wp) return;                                      // (whole waves: Wp = 64 nk)
  const uint32_t w = a.r.work_of[ai];                          // FS_NONE: padding
  const uint64_t bits = __ballot(w < a.r.n_works && a.when[w] != kOut);
  if ((threadIdx.x & 63) == 0) a.pbits[ai >> 6] = bits;
}

// blockIdx.y = row of the planes, a lane per work of the file
__global__ __launch_bounds__(kRunBlock) void k_trd_labels(TrdArgs a) {
  __shared__ uint32_t s_w[kRunBlock / 64];
  const uint32_t r = blockIdx.y;
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  uint32_t x = 0;
  if (w < a.r.n_works) {
    const uint32_t mine = a.when[w];
    if (mine != kOut) {
      x = mine;
      if (r < a.P) {
        const uint32_t h = fs_work_hash(a.term, r, (uint32_t)w);
        x = a.pool_x[(uint32_t)(((uint64_t)h * a.N) >> 32)];   // (below N: h < 2^32)
      }
      if (a.flag && a.flag[w]) {
        const size_t at = (size_t)r * a.Wp + a.r.act[w];
        a.lo[at] = (uint8_t)(x & 127u);
        a.hi[at] = (uint8_t)(x >> 7);
      }
    }
  }
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x) return;
  x = 0;
  for (uint32_t v = 0; v < kRunBlock / 64; ++v) x += s_w[v];
  if (x) atomicAdd(&a.xr[r], x);
}

// sixteen bits to sixteen bytes of 0 / 1: bit i of a nibble lands in byte i
__device__ inline v4i spread16(uint32_t x) {
  v4i f;
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d)
    f[d] = (int)((((x >> (4 * d)) & 0xFu) * 0x00204081u) & 0x01010101u);
  return f;
}

// blockIdx.x = tile of 64 units, blockIdx.y = 128 rows; wave w the 32 rows
// (4 blockIdx.y + w) * 32 ..., as far as the padded rows go.  blockIdx.z = a share of the words k
// when the tiles alone would leave most of the device idle (ksplit > 1): the shares are then
// added into the sums, which the host has cleared
__global__ __launch_bounds__(kProd) void k_trd_product(TrdArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t n_rt = a.Rp / 16;
  const uint32_t rt0 = (blockIdx.y * (kProd / 64) + wave) * kRT;
  if (rt0 >= n_rt) return;
  const uint32_t nt = n_rt - rt0 < kRT ? n_rt - rt0 : kRT;
  const uint32_t nk = a.m.nk;
  const uint32_t kper = (nk + a.ksplit - 1) / a.ksplit;
  const uint32_t k0 = blockIdx.z * kper;
  if (k0 >= nk) return;
  const uint32_t k1 = nk - k0 < kper ? nk : k0 + kper;
  const uint32_t col = lane & 15, grp = lane >> 4;
  const unsigned long long* mw = a.m.cov + (size_t)blockIdx.x * nk * kTile + col;
  const size_t at = (size_t)(rt0 * 16 + col) * a.Wp + grp * 16;
  const uint8_t* pl = a.lo + at;
  const uint8_t* ph = a.hi + at;
  v4i lo[kRT][kUT], hi[kRT][kUT];
#pragma unroll
  for (uint32_t i = 0; i < kRT; ++i)
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j) lo[i][j] = hi[i][j] = v4i{0, 0, 0, 0};
  for (uint32_t k = k0; k < k1; ++k) {
    v4i bf[kUT];
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j)
      bf[j] = spread16((uint32_t)(mw[(size_t)k * kTile + 16 * j] >> (16 * grp)) & 0xFFFFu);
#pragma unroll
    for (uint32_t i = 0; i < kRT; ++i) {
      if (i >= nt) break;
      const size_t off = (size_t)i * 16 * a.Wp + (size_t)k * 64;
      const v4i al = *reinterpret_cast<const v4i*>(pl + off);
      const v4i ah = *reinterpret_cast<const v4i*>(ph + off);
#pragma unroll
      for (uint32_t j = 0; j < kUT; ++j) {
        lo[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bf[j], lo[i][j], 0, 0, 0);
        hi[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bf[j], hi[i][j], 0, 0, 0);
      }
    }
  }
  // D: column lane & 15 is the unit, rows 4 (lane >> 4) .. + 3 are four adjacent rows of a plane
#pragma unroll
  for (uint32_t i = 0; i < kRT; ++i) {
    if (i >= nt) break;
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j) {
      const size_t u = (size_t)blockIdx.x * kTile + 16 * j + col;
      uint32_t* out = a.sums + u * a.Rp + (rt0 + i) * 16 + grp * 4;
      const v4i s = lo[i][j] + hi[i][j] * 128;
      if (a.ksplit == 1) {
        *reinterpret_cast<v4i*>(out) = s;
      } else {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
          if (s[r]) atomicAdd(out + r, (uint32_t)s[r]);
      }
    }
  }
}

// blockIdx.x = unit (padded), blockIdx.y * kRunBlock + threadIdx.x = row (padded)
__global__ __launch_bounds__(kRunBlock) void k_trd_plain(TrdArgs a) {
  const uint32_t b = blockIdx.y * kRunBlock + threadIdx.x;
  if (b >= a.Rp) return;
  const size_t u = blockIdx.x;
  const unsigned long long* row = a.m.cov + (u / kTile) * a.m.nk * kTile + u % kTile;
  const uint8_t* pl = a.lo + (size_t)b * a.Wp;
  const uint8_t* ph = a.hi + (size_t)b * a.Wp;
  uint32_t c = 0;
  for (uint32_t k = 0; k < a.m.nk; ++k) {
    unsigned long long x = row[(size_t)k * kTile];
    while (x) {
      const uint32_t at = k * 64 + (uint32_t)__builtin_ctzll(x);
      c += pl[at] + 128u * ph[at];
      x &= x - 1;
    }
  }
  a.sums[u * a.Rp + b] = c;
}

// a wave per unit
__global__ __launch_bounds__(kRunBlock) void k_trd_sweep(TrdArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t u = blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (u >= a.n_units) return;
  // t, and the smallest and largest observed offset: lane j looks at work 64 k + j of word k
  const unsigned long long* mrow = a.m.cov + (size_t)(u / kTile) * a.m.nk * kTile + u % kTile;
  const uint8_t* pl = a.lo + (size_t)a.P * a.Wp;
  const uint8_t* ph = a.hi + (size_t)a.P * a.Wp;
  uint32_t t = 0, first = FS_NONE, last = 0;
  for (uint32_t k = 0; k < a.m.nk; ++k) {
    const unsigned long long m = mrow[(size_t)k * kTile] & a.pbits[k];
    t += (uint32_t)__popcll(m);
    if ((m >> lane) & 1ull) {
      const uint32_t x = pl[k * 64 + lane] + 128u * ph[k * 64 + lane];
      first = x < first ? x : first;
      last = x > last ? x : last;
    }
  }
  first = ~wave_max(~first);
  last = wave_max(last);
  const uint32_t* row = a.sums + (size_t)u * a.Rp;
  const uint32_t s = row[a.P];
  const int64_t D = (int64_t)s * a.N - (int64_t)t * a.xr[a.P];
  const uint64_t absD = trd_abs(D);
  const uint64_t den = trd_isqrt(((uint64_t)t * (a.N - t)) << 20);
  const bool family = t >= a.min_quoting && t < a.N;         // (so den > 0)
  uint32_t ge = 0;
  for (uint32_t r = lane; r < a.P; r += 64) {
    const uint64_t ad = trd_abs((int64_t)row[r] * a.N - (int64_t)t * a.xr[r]);
    ge += ad >= absD;
    if (!family || !ad) continue;
    const unsigned long long z = (ad << 10) / den;
    if (z && z > a.mx[r]) atomicMax(&a.mx[r], z);
  }
  ge = wave_sum(ge);
  if (lane) return;
  fs_trends_unit* v = a.units + u;
  v->quoting = t;
  v->ge = ge;
  v->adj_ge = FS_NONE;
  v->first_x = t ? first : FS_NONE;
  v->last_x = t ? last : FS_NONE;
  v->reserved = 0u;
  v->offset_sum = s;
  v->statistic = den ? (absD << 10) / den : 0ull;
  v->d = D;
}

// blockIdx.x = kAdjUnits units, a wave per unit in turn
__global__ __launch_bounds__(kRunBlock) void k_trd_adjust(TrdArgs a) {
  __shared__ unsigned long long s_mx[kMaxPerms];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t r = threadIdx.x; r < a.P; r += kRunBlock) s_mx[r] = a.mx[r];
  __syncthreads();
  const uint32_t u0 = blockIdx.x * kAdjUnits;
  const uint32_t u1 = a.n_units - u0 < kAdjUnits ? a.n_units : u0 + kAdjUnits;
  for (uint32_t u = u0 + wave; u < u1; u += kRunBlock / 64) {
    const uint32_t* row = a.sums + (size_t)u * a.Rp;
    const uint32_t t = a.units[u].quoting;
    if (t < a.min_quoting || t >= a.N) continue;
    const uint64_t den = trd_isqrt(((uint64_t)t * (a.N - t)) << 20);
    const uint64_t Z = a.units[u].statistic;
    uint32_t adj = 0;
    for (uint32_t r = lane; r < a.P; r += 64) {
      const uint64_t ad = trd_abs((int64_t)row[r] * a.N - (int64_t)t * a.xr[r]);
      adj += s_mx[r] >= Z;
      if ((ad << 10) / den == s_mx[r]) atomicMin(&a.mu[r], u);
    }
    adj = wave_sum(adj);
    if (lane == 0) a.units[u].adj_ge = adj;
  }
}

// one lane per re-dating
__global__ __launch_bounds__(kRunBlock) void k_trd_perms(TrdArgs a) {
  const uint32_t r = blockIdx.x * kRunBlock + threadIdx.x;
  if (r >= a.P) return;
  const unsigned long long z = a.mx[r];
  reinterpret_cast<uint4*>(a.perms)[r] =
      make_uint4((uint32_t)z, (uint32_t)(z >> 32), a.xr[r], a.mu[r]);
}

// one lane per unit, when no work is active: nobody quotes it under any dating
__global__ __launch_bounds__(kRunBlock) void k_trd_none(TrdArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u >= a.n_units) return;
  uint4* p = reinterpret_cast<uint4*>(a.units + u);
  p[0] = make_uint4(0u, a.P, FS_NONE, FS_NONE);
  p[1] = make_uint4(FS_NONE, 0u, 0u, 0u);
  p[2] = make_uint4(0u, 0u, 0u, 0u);
}

// pool and incidence, labels, product, sweeps, their total
thread_local double t_ms[5];

struct TrdJob {
  IncJob inc;
  DBuf<uint32_t> tally, inpool, pos, sums, xr, mu;
  DBuf<uint16_t> pool_x;
  DBuf<unsigned long long> pbits, mx;
  DBuf<uint8_t> planes;
  Clock<5> clk;
  TrdArgs a{};

  // d_units and d_perms written, and h_sums (host, [n_units][permutations]) unless null (all
  // on `s`, finished on return)
  int run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
          const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
          const uint16_t* d_when, uint32_t min_quoting, uint32_t permutations, uint64_t seed,
          fs_trends_unit* d_units, fs_trends_perm* d_perms, uint32_t* h_sums, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    const uint32_t mfma = env_u32("FS_TRENDS_MFMA", kMfmaDefault, 1u);
    const uint64_t max_bytes =
        env_u32("FS_TRENDS_MAX_BYTES", FS_TRENDS_MAX_BYTES, FS_TRENDS_MAX_BYTES);
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.P = permutations;
    a.R = permutations + 1;
    a.Rp = (a.R + 15) / 16 * 16;
    a.min_quoting = min_quoting;
    a.term = seed * 0x9E3779B97F4A7C15ull;
    a.when = d_when;
    a.units = d_units;
    a.perms = d_perms;
    const dim3 blk(kRunBlock);
    // the check of the offsets rides in front of number(), which waits and refuses after it
    uint32_t st[2] = {0, 0};                                 // a bad offset, N
    FS_TRY(tally.reserve(2));
    FS_TRY(inpool.reserve(n_works));
    FS_TRY(pos.reserve(n_works));
    FS_HIP(hipMemsetAsync(tally.p, 0, sizeof st, s));
    FS_TRY(clk.mark(0, s));
    if (n_works) {
      hipLaunchKernelGGL(k_trd_when, dim3(blocks_of(n_works, kRunBlock)), blk, 0, s, d_when,
                         n_works, inpool.p, tally.p);
      hipLaunchKernelGGL(k_pairs_scan<uint32_t>, dim3(1), dim3(kScanBlock), 0, s, inpool.p,
                         (uint64_t)n_works, pos.p, tally.p + 1);
    }
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(st, tally.p, sizeof st, hipMemcpyDeviceToHost, s));
    int rc = FS_OK;
    if (n)
      rc = inc.number(d_rows, a, max_gap, s);
    else
      FS_HIP(hipStreamSynchronize(s));
    if (st[0]) {
      fs_set_error("a `when` above %u that is not 0xFFFF (a work outside the pool)",
                   FS_TRENDS_MAX_SPAN - 1u);
      return FS_E_INVALID;
    }
    if (rc != FS_OK) return rc;
    a.N = st[1];
    a.pos = pos.p;
    FS_TRY(pool_x.reserve(a.N));
    a.pool_x = pool_x.p;
    if (a.N)
      hipLaunchKernelGGL(k_trd_pool, dim3(blocks_of(n_works, kRunBlock)), blk, 0, s, a);
    const bool some = n && a.r.n_active && n_units;
    FS_TRY(xr.reserve(a.R));
    FS_TRY(mx.reserve(a.P));
    FS_TRY(mu.reserve(a.P));
    FS_HIP(hipMemsetAsync(xr.p, 0, (size_t)a.R * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(mx.p, 0, (size_t)a.P * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(mu.p, 0xFF, (size_t)a.P * sizeof(uint32_t), s));
    a.xr = xr.p;
    a.mx = mx.p;
    a.mu = mu.p;
    size_t rows = 0;
    if (some) {
      rows = (size_t)a.m.n_tiles * kTile;
      const uint64_t mat_bytes = IncJob::mat_bytes(a);
      const uint64_t plane_bytes = 2 * (uint64_t)a.Rp * a.m.nk * 64;
      const uint64_t sum_bytes = (uint64_t)rows * a.Rp * 4;
      if (mat_bytes + plane_bytes + sum_bytes > max_bytes) {
        fs_set_error("%u units over %u works with a passage in %u re-datings: an incidence "
                     "matrix of %llu bytes, two offset planes of %llu bytes and sums of %llu "
                     "bytes are more than %llu bytes", n_units, a.r.n_active, permutations,
                     (unsigned long long)mat_bytes, (unsigned long long)plane_bytes,
                     (unsigned long long)sum_bytes, (unsigned long long)max_bytes);
        return FS_E_UNSUPPORTED;
      }
      a.Wp = a.m.nk * 64;                                    // the active numbers, padded
      FS_TRY(inc.reserve(a, false, s));
      FS_TRY(pbits.reserve(a.m.nk));
      FS_TRY(planes.reserve((size_t)plane_bytes));
      FS_TRY(sums.reserve(rows * a.Rp));
      FS_HIP(hipMemsetAsync(planes.p, 0, (size_t)plane_bytes, s));
      a.pbits = pbits.p;
      a.lo = planes.p;
      a.hi = planes.p + (size_t)plane_bytes / 2;
      a.sums = sums.p;
      a.flag = inc.cj.flag.p;
      inc.incidence(d_rows, a, s);
      hipLaunchKernelGGL(k_trd_pbits, dim3(blocks_of(a.Wp, kRunBlock)), blk, 0, s, a);
    }
    FS_TRY(clk.mark(1, s));
    if (n_works && a.N)
      hipLaunchKernelGGL(k_trd_labels, dim3(blocks_of(n_works, kRunBlock), a.R), blk, 0, s, a);
    FS_TRY(clk.mark(2, s));
    if (some) {
      if (mfma) {
        // few tiles: the words k are shared out (inc_ksplit)
        const uint32_t gy = (a.Rp / 16 + 4 * kRT - 1) / (4 * kRT);
        a.ksplit = inc_ksplit("FS_TRENDS_KSPLIT", (uint64_t)a.m.n_tiles * gy, a.m.nk);
        if (a.ksplit > 1)
          FS_HIP(hipMemsetAsync(sums.p, 0, rows * a.Rp * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_trd_product, dim3(a.m.n_tiles, gy, a.ksplit), dim3(kProd), 0, s, a);
      } else
        hipLaunchKernelGGL(k_trd_plain, dim3((uint32_t)rows, blocks_of(a.Rp, kRunBlock)), blk, 0,
                           s, a);
    }
    FS_TRY(clk.mark(3, s));
    if (some) {
      hipLaunchKernelGGL(k_trd_sweep, dim3(blocks_of(n_units, kRunBlock / 64)), blk, 0, s, a);
      hipLaunchKernelGGL(k_trd_adjust, dim3(blocks_of(n_units, kAdjUnits)), blk, 0, s, a);
    } else if (n_units) {
      hipLaunchKernelGGL(k_trd_none, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s, a);
    }
    hipLaunchKernelGGL(k_trd_perms, dim3(blocks_of(a.P, kRunBlock)), blk, 0, s, a);
    FS_TRY(clk.mark(4, s));
    FS_HIP(hipGetLastError());
    if (h_sums && n_units) {
      if (some)
        FS_HIP(hipMemcpy2DAsync(h_sums, (size_t)a.P * 4, sums.p, (size_t)a.Rp * 4,
                                (size_t)a.P * 4, n_units, hipMemcpyDeviceToHost, s));
      else
        memset(h_sums, 0, (size_t)n_units * a.P * 4);
    }
    FS_HIP(hipStreamSynchronize(s));
    for (int k = 0; k < 4; ++k) t_ms[k] = clk.elapsed(k, k + 1);
    t_ms[4] = t_ms[0] + t_ms[1] + t_ms[2] + t_ms[3];
    return FS_OK;
  }
};

// the rules both entry points share
int trd_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const void* unit_of,
              uint32_t n_units, uint32_t min_words, const void* when, uint32_t min_quoting,
              uint32_t permutations, const void* units, const void* perms) {
  if (!perms || (n_units && !units) || (n_works && !when) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_quoting == 0) {
    fs_set_error("min_words and min_quoting must be at least 1");
    return FS_E_INVALID;
  }
  if (permutations == 0 || permutations > FS_TRENDS_MAX_PERMUTATIONS) {
    fs_set_error("permutations %u: from 1 to %u", permutations, FS_TRENDS_MAX_PERMUTATIONS);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("trends", n_rows, n_script));
  if (n_works > FS_TRENDS_MAX_WORKS) {
    fs_set_error("n_works %u: trends take up to %u", n_works, FS_TRENDS_MAX_WORKS);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_trends(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                         uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                         uint32_t min_words, uint32_t max_gap, const uint16_t* when,
                         uint32_t min_quoting, uint32_t permutations, uint64_t seed,
                         fs_trends_unit* units, fs_trends_perm* perms, uint32_t* sums) {
  FS_TRY(trd_check(n_rows, n_works, n_script, unit_of, n_units, min_words, when, min_quoting,
                   permutations, units, perms));
  if (n_rows && (!work || !fan_ix || !orig_ix)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_unit_of;
  DBuf<uint16_t> d_when;
  DBuf<fs_trends_unit> d_units;
  DBuf<fs_trends_perm> d_perms;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n && n_units ? n_script : 0, nullptr));
  FS_TRY(d_when.upload(when, n_works, nullptr));
  FS_TRY(d_units.reserve(n_units));
  FS_TRY(d_perms.reserve(permutations));
  TrdJob job;
  FS_TRY(job.run(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap, d_when.p,
                 min_quoting, permutations, seed, d_units.p, d_perms.p, sums, nullptr));
  if (n_units) FS_TRY(copy_out(units, d_units, n_units));
  FS_TRY(copy_out(perms, d_perms, permutations));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_trends_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                              uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                              uint32_t min_words, uint32_t max_gap, const uint16_t* d_when,
                              uint32_t min_quoting, uint32_t permutations, uint64_t seed,
                              fs_trends_unit* d_units, fs_trends_perm* d_perms) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: trends take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(trd_check(n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units, min_words, d_when,
                   min_quoting, permutations, d_units, d_perms));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_when & 1) || ((uintptr_t)d_units & 15) || ((uintptr_t)d_perms & 15)) {
    fs_set_error("d_rows, d_units and d_perms must be 16-byte aligned device pointers, "
                 "d_unit_of 4-byte and d_when 2-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  TrdJob job;
  return job.run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                 min_words, max_gap, d_when, min_quoting, permutations, seed, d_units, d_perms,
                 nullptr, ix->stream);
}

extern "C" int fs_trends_times(double* ms) {
  return times_out(ms, t_ms, 5);
}
