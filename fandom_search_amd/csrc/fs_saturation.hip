// fs_saturation.hip -- `ao3.py saturation`: what a sample of the fan works would show, the
// accumulation curve of the quoted units (fs_saturation, fs_saturation_rows in
// include/fandom_search.h).  In order r work w arrives at time h(r, w) = fs_work_hash(term, r, w),
// a pure function of (seed, r, w); the sample at point c is the works with h < T_c.  Nothing is
// sorted, ranked or scattered.  The first time of a unit in an order, first(r, u) = the smallest
// h(r, w) over the active works quoting u, is a min-product of the unit x work incidence bit
// matrix M of fs_incidence.h and the orders x works matrix of times.
//
// Every output is an integer and every merge an integer min or add, so partial results merge in
// any order.  Separate launches; no workgroup waits on another:
//   incidence        IncJob of fs_incidence.h: M and works(u)
//   k_sat_summary    Q, Q1 and Q2 from works(u): a ballot per wave, one atomic add per count
//   k_sat_sizes      a workgroup per order and slab of works: every work of the file hashed into
//                    a histogram over the points in LDS, one global atomic per non-zero bucket
//   k_sat_scan       a workgroup per order: hist[c][r] summed over c (block_scan), n_r(c) or
//                    S_r(c) in its place
//   k_sat_times      FS_SATURATION_TABLE=1: time[active work][order], the orders padded to 64
//   k_sat_product    the hot path.  A wave takes one unit row and 64 orders at a time, a lane
//                    per order.  64 words of the row are loaded at once, a lane each, and the
//                    non-zero ones taken in turn (a ballot, then a read of that lane), for every
//                    chunk of 64 orders the wave has, so the row is read once; the set bits of a
//                    word are walked by wave-uniform control.  A set bit costs one min against
//                    the work's time: one 256-byte read of the table per wave, four in flight
//                    (a bit that is not there stands in as the first again, which a min does
//                    not see), or the hash made again in the lane.  With few rows the chunks of
//                    orders, and then the words k, are shared among workgroups; shares of k
//                    atomicMin into first
//   k_sat_curve      a wave per 128 units and 64 orders, a lane per order: bucket(first) of the
//                    quoted units into byte counters in LDS, [point][lane], then one global
//                    atomic add per non-zero counter into hist[c][r]
//   k_sat_perms      a lane per order: half_at, ninety_at and all_at along S_r(c)
//   k_sat_points     a workgroup per point: the R values of S_r(c) and of n_r(c) sorted in LDS
//                    (fs_sort.h), the order statistics, MIN, MAX and the sums
//   k_sat_first_out  first without its padding, where the caller asked for it
#include "fs_incidence.h"
#include "fs_sort.h"

namespace {

constexpr uint32_t kProd = 256;               // threads of k_sat_product: four waves, a row each
constexpr uint32_t kChunkBlocks = 2048;       // product workgroups wanted before a wave takes
                                              // more than one chunk of 64 orders
constexpr uint32_t kSlab = 1u << 16;          // works a k_sat_sizes workgroup hashes
constexpr uint32_t kCurveUnits = 128;         // units of a k_sat_curve workgroup: a byte counts them
constexpr uint32_t kStat = 256;               // threads of k_sat_points
constexpr uint32_t kTableDefault = 0;         // FS_SATURATION_TABLE when the environment is silent
constexpr uint32_t kMaxPerms = FS_SATURATION_MAX_PERMUTATIONS;
constexpr uint32_t kMaxPoints = FS_SATURATION_MAX_POINTS;
static_assert(kMaxPoints <= kScanBlock, "k_sat_scan: a thread per point");
static_assert(kCurveUnits < 256, "k_sat_curve: byte counters");

struct SatArgs : IncArgs {
  uint32_t R, Rp, P;            // orders; padded to a multiple of 64; the power of two >= R
  uint32_t K;                   // points
  uint32_t t;                   // R * (100 - level) / 200
  uint32_t ksplit;              // workgroups that share the words k of a unit row
  uint32_t osplit, oc_per;      // ... that share its chunks of 64 orders; chunks to each at most
  uint64_t term;               // seed * 0x9E3779B97F4A7C15
  uint32_t* times;              // [r.n_active][Rp]
  uint32_t* first;              // [n_units][Rp]
  uint32_t* uhist;              // [K][Rp] units first seen at point c + 1, then S_r(c + 1)
  uint32_t* whist;              // [K][Rp] works arriving at point c + 1, then n_r(c + 1)
  uint32_t* sums;               // [4] -, Q, Q1, Q2
  uint32_t* out_first;          // [n_units][R]
  fs_saturation_point* points;
  fs_saturation_perm* perms;
  fs_saturation_summary* summary;
};

// bucket(h, points): include/fandom_search.h
__host__ __device__ inline uint32_t sat_bucket(uint32_t h, uint32_t points) {
  return (uint32_t)((((uint64_t)h + 1u) * points + 0xFFFFFFFFull) >> 32);
}

// a lane per unit
__global__ __launch_bounds__(kRunBlock) void k_sat_summary(SatArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t w = u < a.n_units ? a.m.covered[u] : 0u;
  const uint32_t q = (uint32_t)__popcll(__ballot(w > 0));
  const uint32_t q1 = (uint32_t)__popcll(__ballot(w == 1));
  const uint32_t q2 = (uint32_t)__popcll(__ballot(w == 2));
  if (threadIdx.x & 63) return;
  if (q) atomicAdd(&a.sums[1], q);
  if (q1) atomicAdd(&a.sums[2], q1);
  if (q2) atomicAdd(&a.sums[3], q2);
}

// blockIdx.x = order, blockIdx.y = slab of kSlab works
__global__ __launch_bounds__(kRunBlock) void k_sat_sizes(SatArgs a) {
  __shared__ uint32_t s_h[kMaxPoints];
  const uint32_t r = blockIdx.x;
  for (uint32_t c = threadIdx.x; c < a.K; c += kRunBlock) s_h[c] = 0u;
  __syncthreads();
  const uint64_t w0 = (uint64_t)blockIdx.y * kSlab;
  const uint64_t w1 = a.r.n_works - w0 < kSlab ? a.r.n_works : w0 + kSlab;
  for (uint64_t w = w0 + threadIdx.x; w < w1; w += kRunBlock)
    atomicAdd(&s_h[sat_bucket(fs_work_hash(a.term, r, (uint32_t)w), a.K) - 1u], 1u);
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < a.K; c += kRunBlock) {
    const uint32_t v = s_h[c];
    if (v) atomicAdd(&a.whist[(size_t)c * a.Rp + r], v);
  }
}

// blockIdx.x = order, a thread per point: the inclusive sums over c in place
__global__ __launch_bounds__(kScanBlock) void k_sat_scan(uint32_t* hist, uint32_t K,
                                                         uint32_t Rp) {
  __shared__ uint32_t s_w[kScanBlock / 64];
  const uint32_t c = threadIdx.x;
  const bool in = c < K;
  uint32_t* p = hist + (size_t)(in ? c : 0u) * Rp + blockIdx.x;
  const uint32_t x = in ? *p : 0u;
  uint32_t total;
  const uint32_t pre = block_scan<kScanBlock>(x, s_w, &total);
  if (in) *p = pre + x;
}

// a lane per (active work, padded order)
__global__ __launch_bounds__(kRunBlock) void k_sat_times(SatArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= (uint64_t)a.r.n_active * a.Rp) return;
  const uint32_t ai = (uint32_t)(i / a.Rp), r = (uint32_t)(i % a.Rp);
  a.times[i] = fs_work_hash(a.term, r, a.r.work_of[ai]);
}

// the time of active work ai in the lane's order r
template <bool kTable>
__device__ inline uint32_t sat_time(const SatArgs& a, uint32_t ai, uint32_t r) {
  if constexpr (kTable) {
    return a.times[(size_t)ai * a.Rp + r];
  } else {
    return fs_work_hash(a.term, r, a.r.work_of[ai]);
  }
}

// the smallest time in the lane's order r over the set bits of x, the word of the active works
// base .. base + 63 (x wave-uniform), and m
template <bool kTable>
__device__ inline uint32_t sat_word(const SatArgs& a, unsigned long long x, uint32_t base,
                                    uint32_t r, uint32_t m) {
  while (x) {
    if constexpr (kTable) {
      // up to four set bits, four reads in flight: a missing one is the first again, and
      // min(t, t) = t
      const uint32_t b0 = (uint32_t)__builtin_ctzll(x);
      x &= x - 1;
      const uint32_t b1 = x ? (uint32_t)__builtin_ctzll(x) : b0;
      x &= x - 1;
      const uint32_t b2 = x ? (uint32_t)__builtin_ctzll(x) : b0;
      x &= x - 1;
      const uint32_t b3 = x ? (uint32_t)__builtin_ctzll(x) : b0;
      x &= x - 1;
      const uint32_t t0 = sat_time<true>(a, base + b0, r), t1 = sat_time<true>(a, base + b1, r);
      const uint32_t t2 = sat_time<true>(a, base + b2, r), t3 = sat_time<true>(a, base + b3, r);
      const uint32_t t01 = t0 < t1 ? t0 : t1, t23 = t2 < t3 ? t2 : t3;
      const uint32_t tt = t01 < t23 ? t01 : t23;
      if (tt < m) m = tt;
    } else {
      // the hash is arithmetic: a bit a step, none made twice
      const uint32_t t = sat_time<false>(a, base + (uint32_t)__builtin_ctzll(x), r);
      x &= x - 1;
      if (t < m) m = t;
    }
  }
  return m;
}

// blockIdx.x = four units, wave w the unit 4 blockIdx.x + w.  A wave takes 64 orders at a
// time, a lane each: the chunks blockIdx.y, blockIdx.y + gridDim.y, ... of the padded orders,
// a.oc_per of them at most, and reads the words of its row once for all of them; the running
// minimum of a chunk waits in LDS, [wave][chunk][lane], which no other wave touches.
// blockIdx.z = a share of the words k when the rows alone would leave most of the device idle
// (ksplit > 1): the shares then atomicMin into first, which the host has filled with 0xFFFFFFFF
template <bool kTable>
__global__ __launch_bounds__(kProd) void k_sat_product(SatArgs a) {
  extern __shared__ uint32_t s_min[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t u = blockIdx.x * (kProd / 64) + wave;
  if (u >= a.n_units) return;
  const uint32_t n_oc = a.Rp / 64;
  const uint32_t mine_oc = (n_oc - blockIdx.y + gridDim.y - 1) / gridDim.y;   // <= a.oc_per
  uint32_t* mm = s_min + (size_t)wave * a.oc_per * 64 + lane;
  const uint32_t nk = a.m.nk;
  const uint32_t kper = (nk + a.ksplit - 1) / a.ksplit;
  const uint32_t k0 = blockIdx.z * kper;
  if (k0 >= nk) return;
  const uint32_t k1 = nk - k0 < kper ? nk : k0 + kper;
  const unsigned long long* row = a.m.cov + (size_t)(u / kTile) * nk * kTile + u % kTile;
  for (uint32_t j = 0; j < mine_oc; ++j) mm[j * 64] = FS_NONE;
  for (uint32_t kb = k0; kb < k1; kb += 64) {
    // 64 words of the row, a lane each; the words with a set bit in turn, for every chunk
    const uint32_t k = kb + lane;
    const unsigned long long mine = k < k1 ? row[(size_t)k * kTile] : 0ull;
    const uint32_t lo = (uint32_t)mine, hi = (uint32_t)(mine >> 32);
    const uint64_t some = __ballot(mine != 0ull);
    if (!some) continue;
    for (uint32_t j = 0; j < mine_oc; ++j) {
      const uint32_t r = (blockIdx.y + j * gridDim.y) * 64 + lane;           // < Rp
      uint32_t m = mm[j * 64];
      uint64_t todo = some;
      while (todo) {
        const uint32_t from = (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1;
        const unsigned long long x =
            (unsigned long long)lane_u32(hi, from) << 32 | lane_u32(lo, from);
        m = sat_word<kTable>(a, x, (kb + from) * 64, r, m);
      }
      mm[j * 64] = m;
    }
  }
  for (uint32_t j = 0; j < mine_oc; ++j) {
    const uint32_t r = (blockIdx.y + j * gridDim.y) * 64 + lane;
    const uint32_t m = mm[j * 64];
    uint32_t* out = a.first + (size_t)u * a.Rp + r;
    if (a.ksplit == 1)
      *out = m;
    else if (m != FS_NONE)
      atomicMin(out, m);
  }
}

// blockIdx.x = kCurveUnits units, blockIdx.y = 64 orders; one wave, a lane per order.  Dynamic
// LDS: K * 64 bytes, counter [point][lane]
__global__ __launch_bounds__(64) void k_sat_curve(SatArgs a) {
  extern __shared__ uint32_t s_dyn[];
  uint8_t* s_h = reinterpret_cast<uint8_t*>(s_dyn);
  const uint32_t lane = threadIdx.x;
  const uint32_t r = blockIdx.y * 64 + lane;
  for (uint32_t i = lane; i < a.K * 16; i += 64) s_dyn[i] = 0u;
  __syncthreads();
  const uint32_t u0 = blockIdx.x * kCurveUnits;
  const uint32_t u1 = a.n_units - u0 < kCurveUnits ? a.n_units : u0 + kCurveUnits;
  if (r < a.R) {
    for (uint32_t u = u0; u < u1; ++u) {
      if (a.m.covered[u] == 0) continue;                        // nobody quotes it
      const uint32_t b = sat_bucket(a.first[(size_t)u * a.Rp + r], a.K) - 1u;
      s_h[b * 64 + lane] = (uint8_t)(s_h[b * 64 + lane] + 1u);
    }
    for (uint32_t c = 0; c < a.K; ++c) {
      const uint32_t v = s_h[c * 64 + lane];
      if (v) atomicAdd(&a.uhist[(size_t)c * a.Rp + r], v);
    }
  }
}

// a lane per order, behind k_sat_scan of uhist
__global__ __launch_bounds__(kRunBlock) void k_sat_perms(SatArgs a) {
  const uint32_t r = blockIdx.x * kRunBlock + threadIdx.x;
  if (r >= a.R) return;
  const unsigned long long Q = a.sums[1];
  uint32_t half = 0, ninety = 0, all = 0;
  for (uint32_t c = 1; c <= a.K; ++c) {
    const unsigned long long S = a.uhist[(size_t)(c - 1) * a.Rp + r];
    if (!half && 2 * S >= Q) half = c;
    if (!ninety && 10 * S >= 9 * Q) ninety = c;
    if (!all && S == Q) all = c;
  }
  reinterpret_cast<uint4*>(a.perms)[r] = make_uint4(half, ninety, all, 0u);
}

// blockIdx.x = point - 1: s_c (S_r) and s_p (n_r) ascending over P >= R entries, the padding at
// the top
__global__ __launch_bounds__(kStat) void k_sat_points(SatArgs a) {
  __shared__ uint32_t s_c[kMaxPerms], s_p[kMaxPerms];
  __shared__ unsigned long long s_u[kStat / 64], s_n[kStat / 64];
  const uint32_t c = blockIdx.x, tid = threadIdx.x;
  const uint32_t* ru = a.uhist + (size_t)c * a.Rp;
  const uint32_t* rw = a.whist + (size_t)c * a.Rp;
  unsigned long long usum = 0, wsum = 0;
  for (uint32_t i = tid; i < a.P; i += kStat) {
    uint32_t x = FS_NONE, y = FS_NONE;
    if (i < a.R) {
      x = ru[i];
      y = rw[i];
      usum += x;
      wsum += y;
    }
    s_c[i] = x;
    s_p[i] = y;
  }
  usum = wave_sum(usum);
  wsum = wave_sum(wsum);
  if ((tid & 63) == 0) {
    s_u[tid >> 6] = usum;
    s_n[tid >> 6] = wsum;
  }
  block_sort_two<kStat>(s_c, s_p, a.P);
  if (tid) return;
  usum = wsum = 0;
  for (uint32_t w = 0; w < kStat / 64; ++w) {
    usum += s_u[w];
    wsum += s_n[w];
  }
  const uint32_t lo = a.t, hi = a.R - 1 - a.t, mid = (a.R - 1) / 2;
  fs_saturation_point* v = a.points + c;
  v->units_low = s_c[lo];
  v->units_median = s_c[mid];
  v->units_high = s_c[hi];
  v->units_min = s_c[0];
  v->units_max = s_c[a.R - 1];
  v->works_low = s_p[lo];
  v->works_median = s_p[mid];
  v->works_high = s_p[hi];
  v->units_sum = usum;
  v->works_sum = wsum;
  v->reserved0 = 0ull;
  v->reserved1 = 0ull;
}

// one lane
__global__ void k_sat_final(SatArgs a) {
  if (threadIdx.x || blockIdx.x) return;
  *reinterpret_cast<uint4*>(a.summary) =
      make_uint4(a.r.n_active, a.sums[1], a.sums[2], a.sums[3]);
}

// a lane per (unit, order)
__global__ __launch_bounds__(kRunBlock) void k_sat_first_out(SatArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= (uint64_t)a.n_units * a.R) return;
  const uint32_t u = (uint32_t)(i / a.R), r = (uint32_t)(i % a.R);
  a.out_first[i] = a.first[(size_t)u * a.Rp + r];
}

// incidence, sizes, times, product, curve, points, their total; table read, shares of k
// and of the chunks of orders
thread_local double t_ms[10];

struct SatJob {
  IncJob inc;
  DBuf<uint32_t> times, first, hist, sums;
  Clock<7> clk;
  SatArgs a{};

  // d_works, d_points, d_perms, d_summary and (unless null) d_first written (all on `s`,
  // finished on return)
  int run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
          const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
          uint32_t permutations, uint32_t points, uint64_t seed, uint32_t level,
          uint32_t* d_works, fs_saturation_point* d_points, fs_saturation_perm* d_perms,
          fs_saturation_summary* d_summary, uint32_t* d_first, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    uint32_t table = env_u32("FS_SATURATION_TABLE", kTableDefault, 1u);
    const uint64_t max_bytes =
        env_u32("FS_SATURATION_MAX_BYTES", FS_SATURATION_MAX_BYTES, FS_SATURATION_MAX_BYTES);
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.R = permutations;
    a.Rp = (permutations + 63) / 64 * 64;
    a.P = 1;
    while (a.P < permutations) a.P <<= 1;
    a.K = points;
    a.t = permutations * (100u - level) / 200u;
    a.ksplit = a.osplit = a.oc_per = 1;
    a.term = seed * 0x9E3779B97F4A7C15ull;
    a.out_first = d_first;
    a.points = d_points;
    a.perms = d_perms;
    a.summary = d_summary;
    const size_t hist_words = (size_t)a.K * a.Rp;
    FS_TRY(hist.reserve(2 * hist_words));
    FS_TRY(sums.reserve(4));
    FS_HIP(hipMemsetAsync(hist.p, 0, 2 * hist_words * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(sums.p, 0, 4 * sizeof(uint32_t), s));
    a.uhist = hist.p;
    a.whist = hist.p + hist_words;
    a.sums = sums.p;
    const dim3 blk(kRunBlock);
    if (n) FS_TRY(inc.number(d_rows, a, max_gap, s));
    const bool some = n && a.r.n_active && n_units;
    if (some) {
      const uint64_t mat_bytes = IncJob::mat_bytes(a);
      const uint64_t first_bytes = (uint64_t)n_units * a.Rp * 4;
      const uint64_t hist_bytes = 2ull * hist_words * 4;
      const uint64_t table_bytes = (uint64_t)a.r.n_active * a.Rp * 4;
      if (mat_bytes + first_bytes + hist_bytes > max_bytes) {
        fs_set_error("%u units over %u works with a passage in %u orders and %u points: an "
                     "incidence matrix of %llu bytes, first times of %llu bytes and histograms "
                     "of %llu bytes are more than %llu bytes", n_units, a.r.n_active,
                     permutations, points, (unsigned long long)mat_bytes,
                     (unsigned long long)first_bytes, (unsigned long long)hist_bytes,
                     (unsigned long long)max_bytes);
        return FS_E_UNSUPPORTED;
      }
      // the table of times is the part a call can do without
      if (mat_bytes + first_bytes + hist_bytes + table_bytes > max_bytes) table = 0;
      FS_TRY(inc.reserve(a, true, s));
      FS_TRY(first.reserve((size_t)n_units * a.Rp));
      if (table) FS_TRY(times.reserve((size_t)a.r.n_active * a.Rp));
      a.first = first.p;
      a.times = times.p;
      // A wave reads its row once for all the chunks of 64 orders it takes.  Few rows: the
      // chunks are shared out until there are kChunkBlocks workgroups (FS_SATURATION_OSPLIT:
      // that many shares, for the tests)
      const uint32_t row_blocks = blocks_of(n_units, kProd / 64), n_oc = a.Rp / 64;
      uint32_t osplit = env_u32("FS_SATURATION_OSPLIT", 0u, 64u);
      if (!osplit) osplit = (kChunkBlocks + row_blocks - 1) / row_blocks;
      a.osplit = osplit < n_oc ? osplit : n_oc;
      a.oc_per = (n_oc + a.osplit - 1) / a.osplit;
      // still few workgroups: the words k are shared out (inc_ksplit)
      a.ksplit = inc_ksplit("FS_SATURATION_KSPLIT", (uint64_t)row_blocks * a.osplit, a.m.nk);
      if (a.ksplit > 1)
        FS_HIP(hipMemsetAsync(first.p, 0xFF, (size_t)n_units * a.Rp * sizeof(uint32_t), s));
    }
    FS_TRY(clk.mark(0, s));
    if (some) {
      inc.incidence(d_rows, a, s);
      hipLaunchKernelGGL(k_sat_summary, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s, a);
    }
    FS_TRY(clk.mark(1, s));
    if (n_works)
      hipLaunchKernelGGL(k_sat_sizes, dim3(a.R, blocks_of(n_works, kSlab)), blk, 0, s, a);
    hipLaunchKernelGGL(k_sat_scan, dim3(a.R), dim3(kScanBlock), 0, s, a.whist, a.K, a.Rp);
    FS_TRY(clk.mark(2, s));
    if (some && table)
      hipLaunchKernelGGL(k_sat_times, dim3(blocks_of((uint64_t)a.r.n_active * a.Rp, kRunBlock)),
                         blk, 0, s, a);
    FS_TRY(clk.mark(3, s));
    if (some) {
      const dim3 grid(blocks_of(n_units, kProd / 64), a.osplit, a.ksplit);
      const size_t lds = (size_t)(kProd / 64) * a.oc_per * 64 * sizeof(uint32_t);   // <= 64 KB
      if (table)
        hipLaunchKernelGGL(k_sat_product<true>, grid, dim3(kProd), lds, s, a);
      else
        hipLaunchKernelGGL(k_sat_product<false>, grid, dim3(kProd), lds, s, a);
    }
    FS_TRY(clk.mark(4, s));
    if (some)
      hipLaunchKernelGGL(k_sat_curve, dim3(blocks_of(n_units, kCurveUnits), a.Rp / 64), dim3(64),
                         (size_t)a.K * 64, s, a);
    hipLaunchKernelGGL(k_sat_scan, dim3(a.R), dim3(kScanBlock), 0, s, a.uhist, a.K, a.Rp);
    hipLaunchKernelGGL(k_sat_perms, dim3(blocks_of(a.R, kRunBlock)), blk, 0, s, a);
    FS_TRY(clk.mark(5, s));
    hipLaunchKernelGGL(k_sat_points, dim3(a.K), dim3(kStat), 0, s, a);
    hipLaunchKernelGGL(k_sat_final, dim3(1), dim3(64), 0, s, a);
    FS_HIP(hipGetLastError());
    if (n_units) {
      const size_t first_words = (size_t)n_units * a.R;
      if (some) {
        FS_HIP(hipMemcpyAsync(d_works, a.m.covered, (size_t)n_units * sizeof(uint32_t),
                              hipMemcpyDeviceToDevice, s));
        if (d_first)
          hipLaunchKernelGGL(k_sat_first_out, dim3(blocks_of(first_words, kRunBlock)), blk, 0, s,
                             a);
      } else {
        FS_HIP(hipMemsetAsync(d_works, 0, (size_t)n_units * sizeof(uint32_t), s));
        if (d_first) FS_HIP(hipMemsetAsync(d_first, 0xFF, first_words * sizeof(uint32_t), s));
      }
    }
    FS_TRY(clk.mark(6, s));
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));
    t_ms[6] = 0.0;
    for (int k = 0; k < 6; ++k) {
      t_ms[k] = clk.elapsed(k, k + 1);
      t_ms[6] += t_ms[k];
    }
    t_ms[7] = some && table ? 1.0 : 0.0;
    t_ms[8] = (double)a.ksplit;
    t_ms[9] = (double)a.osplit;
    return FS_OK;
  }
};

// the rules both entry points share
int sat_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const void* unit_of,
              uint32_t n_units, uint32_t min_words, uint32_t permutations, uint32_t points,
              uint32_t level, const void* works, const void* pts, const void* perms,
              const void* summary) {
  if (!pts || !perms || !summary || (n_units && !works) ||
      (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (permutations == 0 || permutations > FS_SATURATION_MAX_PERMUTATIONS) {
    fs_set_error("permutations %u: from 1 to %u", permutations, FS_SATURATION_MAX_PERMUTATIONS);
    return FS_E_INVALID;
  }
  if (points == 0 || points > FS_SATURATION_MAX_POINTS) {
    fs_set_error("points %u: from 1 to %u", points, FS_SATURATION_MAX_POINTS);
    return FS_E_INVALID;
  }
  if (level < 50 || level > 99) {
    fs_set_error("level %u: a whole percentage from 50 to 99", level);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("saturation curves", n_rows, n_script));
  if (n_works > FS_SATURATION_MAX_WORKS) {
    fs_set_error("n_works %u: saturation curves take up to %u", n_works,
                 FS_SATURATION_MAX_WORKS);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_saturation(int device, const uint32_t* work, const uint32_t* fan_ix,
                             const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                             uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                             uint32_t min_words, uint32_t max_gap, uint32_t permutations,
                             uint32_t points, uint64_t seed, uint32_t level, uint32_t* works,
                             fs_saturation_point* pts, fs_saturation_perm* perms,
                             fs_saturation_summary* summary, uint32_t* first) {
  FS_TRY(sat_check(n_rows, n_works, n_script, unit_of, n_units, min_words, permutations, points,
                   level, works, pts, perms, summary));
  if (n_rows && (!work || !fan_ix || !orig_ix)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  const size_t first_words = first ? (size_t)n_units * permutations : 0;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_unit_of, d_works, d_first;
  DBuf<fs_saturation_point> d_points;
  DBuf<fs_saturation_perm> d_perms;
  DBuf<fs_saturation_summary> d_summary;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n && n_units ? n_script : 0, nullptr));
  FS_TRY(d_works.reserve(n_units));
  FS_TRY(d_points.reserve(points));
  FS_TRY(d_perms.reserve(permutations));
  FS_TRY(d_summary.reserve(1));
  if (first) FS_TRY(d_first.reserve(first_words));
  SatJob job;
  FS_TRY(job.run(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap,
                 permutations, points, seed, level, d_works.p, d_points.p, d_perms.p,
                 d_summary.p, first ? d_first.p : nullptr, nullptr));
  if (n_units) FS_TRY(copy_out(works, d_works, n_units));
  FS_TRY(copy_out(pts, d_points, points));
  FS_TRY(copy_out(perms, d_perms, permutations));
  FS_TRY(copy_out(summary, d_summary, 1));
  if (first_words) FS_TRY(copy_out(first, d_first, first_words));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_saturation_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                  uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                                  uint32_t min_words, uint32_t max_gap, uint32_t permutations,
                                  uint32_t points, uint64_t seed, uint32_t level,
                                  uint32_t* d_works, fs_saturation_point* d_points,
                                  fs_saturation_perm* d_perms, fs_saturation_summary* d_summary,
                                  uint32_t* d_first) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: saturation curves take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(sat_check(n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units, min_words,
                   permutations, points, level, d_works, d_points, d_perms, d_summary));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_works & 3) || ((uintptr_t)d_first & 3) || ((uintptr_t)d_points & 15) ||
      ((uintptr_t)d_perms & 15) || ((uintptr_t)d_summary & 15)) {
    fs_set_error("d_rows, d_points, d_perms and d_summary must be 16-byte aligned device "
                 "pointers, d_unit_of, d_works and d_first 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  SatJob job;
  return job.run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                 min_words, max_gap, permutations, points, seed, level, d_works, d_points,
                 d_perms, d_summary, d_first, ix->stream);
}

extern "C" int fs_saturation_times(double* ms) {
  return times_out(ms, t_ms, 10);
}

extern "C" uint32_t fs_saturation_bucket(uint32_t h, uint32_t points) {
  return sat_bucket(h, points);
}
