// fs_intervals.hip -- `ao3.py intervals`: how sure the works-per-unit counts are, a Poisson
// bootstrap over the fan works (fs_intervals, fs_intervals_rows in include/fandom_search.h).
// Every work gets a multiplicity m(b, w) in each of B replicates, a pure function of (seed, b, w);
// the recount of every unit in every replicate is one product, counts = M x mult^T, of the unit x
// work incidence bit matrix M of fs_incidence.h and the B x works matrix of multiplicity bytes.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   incidence        IncJob of fs_incidence.h: M and works(u)
//   k_int_totals     a workgroup per replicate: N_b over every work of the file, A_b over the
//                    active ones
//   k_int_mult       a lane per four bytes of mult[b][active work], replicate-major, the rows
//                    padded to 16 replicates and 64 works with zeros
//   k_int_product    the hot path: v_mfma_i32_16x16x64_i8.  A workgroup takes a tile of 64 units
//                    and 256 replicates, each of its four waves 64 units x 64 replicates: per
//                    64-bit word k of M four B fragments (16 units each), expanded once from bits
//                    to 0/1 bytes, against four A fragments (16 replicates x 64 works of mult, 16
//                    bytes a lane straight from memory), sixteen MFMAs an expansion.  With few
//                    tiles the words k are shared among workgroups that add into counts
//   k_int_plain      FS_INTERVALS_MFMA=0: a lane per (unit, replicate) walks the set bits of the
//                    unit's row; no matrix instruction.  For the tests and the bench's A/B
//   k_int_stats      a workgroup per unit: its B counts and its B ppm values sorted in LDS (a
//                    bitonic network over the next power of two, fs_sort.h), the three order
//                    statistics of each and the sum
//   k_int_quoted     Q_b: lanes over replicates, waves over units, one atomic add per workgroup
//                    and replicate
//   (host)           works(u) copied back, the observed order by a stable sort, rank and next up
//   k_int_units      a wave per unit: AHEAD / TIED / BEHIND from its row and its neighbour's
//   k_int_reps       a lane per replicate: its fs_interval_replicate
//
// The fragment maps.  The sum over k is the same under any assignment of k to (lane group,
// element) as long as A and B use the same one, and both take byte j of lane group g as work
// 64 k + 16 g + j.  What is relied on: row = lane & 15 for A (the replicate), column =
// lane & 15 for B (the unit), and the C/D map col = lane & 15, row = 4 * (lane >> 4) + reg.
#include "fs_incidence.h"
#include "fs_sort.h"

#include <algorithm>
#include <vector>

namespace {

constexpr uint32_t kProd = 256;               // threads of k_int_product: four waves
constexpr uint32_t kUT = 4;                   // B fragments (16 units) a wave holds: a tile of M
constexpr uint32_t kRT = 4;                   // A fragments (16 replicates) against each of them
constexpr uint32_t kStat = 256;              // threads of k_int_stats
constexpr uint32_t kMaxReps = FS_INTERVALS_MAX_REPLICATES;

typedef int v4i __attribute__((ext_vector_type(4)));

struct IntArgs : IncArgs {
  uint32_t B, Bp, P;            // replicates; padded to a multiple of 16; the power of two >= B
  uint32_t Wp;                  // bytes of a row of mult: m.nk * 64
  uint32_t t;                   // B * (100 - level) / 200
  uint32_t ksplit;              // workgroups that share the words k of a product tile
  uint64_t term;                // seed * 0x9E3779B97F4A7C15
  const uint32_t* flag;         // [r.n_works] 1: active (null: no records)
  uint8_t* mult;                // [Bp][Wp]
  uint32_t* counts;             // [m.n_tiles * 64][Bp]
  uint32_t* tot;                // [3][Bp]: N_b, A_b, Q_b
  const uint32_t* rank;         // [n_units]
  const uint32_t* next;         // [n_units]
  fs_interval_unit* units;
  fs_interval_replicate* reps;
};

// m(b, w): include/fandom_search.h
__host__ __device__ inline uint32_t int_mult(uint64_t term, uint32_t b, uint32_t w) {
  const uint32_t h = fs_work_hash(term, b, w);
  return (h >= 1580030168u) + (h >= 3160060337u) + (h >= 3950075421u) + (h >= 4213413783u) +
         (h >= 4279248373u) + (h >= 4292415291u) + (h >= 4294609777u) + (h >= 4294923276u) +
         (h >= 4294962463u) + (h >= 4294966817u) + (h >= 4294967252u) + (h >= 4294967292u) +
         (h >= 4294967295u);
}

// blockIdx.x = replicate
__global__ __launch_bounds__(kRunBlock) void k_int_totals(IntArgs a) {
  __shared__ uint32_t s_n[kRunBlock / 64], s_a[kRunBlock / 64];
  const uint32_t b = blockIdx.x;
  uint32_t all = 0, act = 0;
  for (uint32_t w = threadIdx.x; w < a.r.n_works; w += kRunBlock) {
    const uint32_t m = int_mult(a.term, b, w);
    all += m;
    if (a.flag && a.flag[w]) act += m;
  }
  all = wave_sum(all);
  act = wave_sum(act);
  if ((threadIdx.x & 63) == 0) {
    s_n[threadIdx.x >> 6] = all;
    s_a[threadIdx.x >> 6] = act;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    all = act = 0;
    for (uint32_t w = 0; w < kRunBlock / 64; ++w) {
      all += s_n[w];
      act += s_a[w];
    }
    a.tot[b] = all;
    a.tot[a.Bp + b] = act;
  }
}

// a lane per four adjacent active works of a replicate, the padding included
__global__ __launch_bounds__(kRunBlock) void k_int_mult(IntArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  const uint32_t per = a.Wp / 4;
  if (i >= (uint64_t)a.Bp * per) return;
  const uint32_t b = (uint32_t)(i / per), q = (uint32_t)(i % per);
  uint32_t v = 0;
  if (b < a.B) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t ai = q * 4 + j;
      if (ai < a.r.n_active) v |= int_mult(a.term, b, a.r.work_of[ai]) << (8 * j);
    }
  }
  reinterpret_cast<uint32_t*>(a.mult)[i] = v;
}

// sixteen bits to sixteen bytes of 0 / 1: bit i of a nibble lands in byte i
__device__ inline v4i spread16(uint32_t x) {
  v4i f;
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d)
    f[d] = (int)((((x >> (4 * d)) & 0xFu) * 0x00204081u) & 0x01010101u);
  return f;
}

// blockIdx.x = tile of 64 units, blockIdx.y = 256 replicates; wave w the 64 replicates
// (4 blockIdx.y + w) * 64 ..., as far as the padded replicates go.  blockIdx.z = a share of the
// words k when the tiles alone would leave most of the device idle (ksplit > 1): the shares are
// then added into counts, which the host has cleared
__global__ __launch_bounds__(kProd) void k_int_product(IntArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t n_rt = a.Bp / 16;
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
  const uint8_t* ma = a.mult + (size_t)(rt0 * 16 + col) * a.Wp + grp * 16;
  v4i acc[kRT][kUT];
#pragma unroll
  for (uint32_t i = 0; i < kRT; ++i)
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j) acc[i][j] = v4i{0, 0, 0, 0};
  for (uint32_t k = k0; k < k1; ++k) {
    v4i bf[kUT];
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j)
      bf[j] = spread16((uint32_t)(mw[(size_t)k * kTile + 16 * j] >> (16 * grp)) & 0xFFFFu);
#pragma unroll
    for (uint32_t i = 0; i < kRT; ++i) {
      if (i >= nt) break;
      const v4i af = *reinterpret_cast<const v4i*>(ma + (size_t)i * 16 * a.Wp + (size_t)k * 64);
#pragma unroll
      for (uint32_t j = 0; j < kUT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[j], acc[i][j], 0, 0, 0);
    }
  }
  // D: column lane & 15 is the unit, rows 4 (lane >> 4) .. + 3 are four adjacent replicates
#pragma unroll
  for (uint32_t i = 0; i < kRT; ++i) {
    if (i >= nt) break;
#pragma unroll
    for (uint32_t j = 0; j < kUT; ++j) {
      const size_t u = (size_t)blockIdx.x * kTile + 16 * j + col;
      uint32_t* out = a.counts + u * a.Bp + (rt0 + i) * 16 + grp * 4;
      if (a.ksplit == 1) {
        *reinterpret_cast<v4i*>(out) = acc[i][j];
      } else {
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r)
          if (acc[i][j][r]) atomicAdd(out + r, (uint32_t)acc[i][j][r]);
      }
    }
  }
}

// blockIdx.x = unit (padded), blockIdx.y * kRunBlock + threadIdx.x = replicate (padded)
__global__ __launch_bounds__(kRunBlock) void k_int_plain(IntArgs a) {
  const uint32_t b = blockIdx.y * kRunBlock + threadIdx.x;
  if (b >= a.Bp) return;
  const size_t u = blockIdx.x;
  const unsigned long long* row = a.m.cov + (u / kTile) * a.m.nk * kTile + u % kTile;
  const uint8_t* mb = a.mult + (size_t)b * a.Wp;
  uint32_t c = 0;
  for (uint32_t k = 0; k < a.m.nk; ++k) {
    unsigned long long x = row[(size_t)k * kTile];
    while (x) {
      c += mb[k * 64 + (uint32_t)__builtin_ctzll(x)];
      x &= x - 1;
    }
  }
  a.counts[u * a.Bp + b] = c;
}

// blockIdx.x = unit: s_c and s_p ascending over P >= B entries, the padding at the top
__global__ __launch_bounds__(kStat) void k_int_stats(IntArgs a) {
  __shared__ uint32_t s_c[kMaxReps], s_p[kMaxReps];
  __shared__ unsigned long long s_w[kStat / 64];
  const uint32_t u = blockIdx.x, tid = threadIdx.x;
  const uint32_t* row = a.counts + (size_t)u * a.Bp;
  unsigned long long sum = 0;
  for (uint32_t i = tid; i < a.P; i += kStat) {
    uint32_t c = FS_NONE, p = FS_NONE;
    if (i < a.B) {
      c = row[i];
      const uint32_t n = a.tot[i];
      p = (uint32_t)((unsigned long long)c * 1000000ull / (n ? n : 1u));
      sum += c;
    }
    s_c[i] = c;
    s_p[i] = p;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) s_w[tid >> 6] = sum;
  block_sort_two<kStat>(s_c, s_p, a.P);
  if (tid) return;
  sum = 0;
  for (uint32_t w = 0; w < kStat / 64; ++w) sum += s_w[w];
  fs_interval_unit* v = a.units + u;
  const uint32_t lo = a.t, hi = a.B - 1 - a.t, mid = (a.B - 1) / 2;
  v->works = a.m.covered[u];
  v->works_low = s_c[lo];
  v->works_median = s_c[mid];
  v->works_high = s_c[hi];
  v->ppm_low = s_p[lo];
  v->ppm_median = s_p[mid];
  v->ppm_high = s_p[hi];
  v->mean_milli = sum * 1000ull / a.B;
}

// blockIdx.x = 256 units, blockIdx.y = 64 replicates: a lane is a replicate, wave w takes the
// units w, w + 4, ...
__global__ __launch_bounds__(kRunBlock) void k_int_quoted(IntArgs a) {
  __shared__ uint32_t s_q[kRunBlock / 64][64];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t b = blockIdx.y * 64 + lane;
  const uint32_t u0 = blockIdx.x * kRunBlock;
  const uint32_t u1 = a.n_units - u0 < kRunBlock ? a.n_units : u0 + kRunBlock;
  uint32_t q = 0;
  if (b < a.B)
    for (uint32_t u = u0 + wave; u < u1; u += kRunBlock / 64)
      q += a.counts[(size_t)u * a.Bp + b] != 0;
  s_q[wave][lane] = q;
  __syncthreads();
  if (wave || b >= a.B) return;
  q = 0;
  for (uint32_t w = 0; w < kRunBlock / 64; ++w) q += s_q[w][lane];
  if (q) atomicAdd(&a.tot[2 * a.Bp + b], q);
}

// a wave per unit
__global__ __launch_bounds__(kRunBlock) void k_int_units(IntArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t u = blockIdx.x * (kRunBlock / 64) + (threadIdx.x >> 6);
  if (u >= a.n_units) return;
  const uint32_t nx = a.next[u];
  uint32_t ahead = 0, tied = 0, behind = 0;
  if (nx < a.n_units) {
    const uint32_t* mine = a.counts + (size_t)u * a.Bp;
    const uint32_t* theirs = a.counts + (size_t)nx * a.Bp;
    for (uint32_t b = lane; b < a.B; b += 64) {
      const uint32_t x = mine[b], y = theirs[b];
      ahead += x > y;
      tied += x == y;
      behind += x < y;
    }
  }
  ahead = wave_sum(ahead);
  tied = wave_sum(tied);
  behind = wave_sum(behind);
  if (lane) return;
  fs_interval_unit* v = a.units + u;
  const uint32_t nw = a.r.n_works ? a.r.n_works : 1u;
  v->ppm = (uint32_t)((unsigned long long)a.m.covered[u] * 1000000ull / nw);
  v->rank = a.rank[u];
  v->next = nx < a.n_units ? nx : FS_NONE;
  v->ahead = ahead;
  v->tied = tied;
  v->behind = behind;
  v->reserved = 0u;
}

// one lane per unit, when no work is active: nobody quotes it in any replicate, the observed
// order is the units' own
__global__ __launch_bounds__(kRunBlock) void k_int_none(IntArgs a) {
  const uint64_t u = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (u >= a.n_units) return;
  const bool last = u + 1 == a.n_units;
  uint4* p = reinterpret_cast<uint4*>(a.units + u);
  p[0] = make_uint4(0u, 0u, 0u, 0u);
  p[1] = make_uint4(0u, 0u, 0u, 0u);
  p[2] = make_uint4(1u, last ? FS_NONE : (uint32_t)u + 1u, 0u, last ? 0u : a.B);
  p[3] = make_uint4(0u, 0u, 0u, 0u);
}

// one lane per replicate
__global__ __launch_bounds__(kRunBlock) void k_int_reps(IntArgs a) {
  const uint32_t b = blockIdx.x * kRunBlock + threadIdx.x;
  if (b >= a.B) return;
  reinterpret_cast<uint4*>(a.reps)[b] =
      make_uint4(a.tot[b], a.tot[a.Bp + b], a.tot[2 * a.Bp + b], 0u);
}

// incidence, multiplicities, product, statistics, neighbours, their total
thread_local double t_ms[6];

struct IntJob {
  IncJob inc;
  DBuf<uint32_t> counts, tot, order;
  DBuf<uint8_t> mult;
  Clock<6> clk;
  IntArgs a{};

  // d_units and d_reps written (all on `s`, finished on return)
  int run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
          const uint32_t* d_unit_of, uint32_t n_units, uint32_t min_words, uint32_t max_gap,
          uint32_t replicates, uint64_t seed, uint32_t level, fs_interval_unit* d_units,
          fs_interval_replicate* d_reps, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    const uint32_t mfma = env_u32("FS_INTERVALS_MFMA", 1u, 1u);
    const uint64_t max_bytes =
        env_u32("FS_INTERVALS_MAX_BYTES", FS_INTERVALS_MAX_BYTES, FS_INTERVALS_MAX_BYTES);
    IncJob::set(a, n, n_works, n_script, min_words, d_unit_of, n_units);
    a.B = replicates;
    a.Bp = (replicates + 15) / 16 * 16;
    a.P = 1;
    while (a.P < replicates) a.P <<= 1;
    a.t = replicates * (100u - level) / 200u;
    a.term = seed * 0x9E3779B97F4A7C15ull;
    a.units = d_units;
    a.reps = d_reps;
    FS_TRY(tot.reserve(3 * (size_t)a.Bp));
    FS_HIP(hipMemsetAsync(tot.p, 0, 3 * (size_t)a.Bp * sizeof(uint32_t), s));
    a.tot = tot.p;
    const dim3 blk(kRunBlock);
    if (n) {
      FS_TRY(inc.number(d_rows, a, max_gap, s));
      a.flag = inc.cj.flag.p;
    }
    const bool some = n && a.r.n_active && n_units;
    size_t rows = 0;
    if (some) {
      rows = (size_t)a.m.n_tiles * kTile;
      const uint64_t mat_bytes = IncJob::mat_bytes(a);
      const uint64_t mult_bytes = (uint64_t)a.Bp * a.m.nk * 64;
      const uint64_t count_bytes = (uint64_t)rows * a.Bp * 4;
      if (mat_bytes + mult_bytes + count_bytes > max_bytes) {
        fs_set_error("%u units over %u works with a passage in %u replicates: an incidence "
                     "matrix of %llu bytes, multiplicities of %llu bytes and counts of %llu "
                     "bytes are more than %llu bytes", n_units, a.r.n_active, replicates,
                     (unsigned long long)mat_bytes, (unsigned long long)mult_bytes,
                     (unsigned long long)count_bytes, (unsigned long long)max_bytes);
        return FS_E_UNSUPPORTED;
      }
      a.Wp = a.m.nk * 64;                                  // the active numbers, padded
      FS_TRY(inc.reserve(a, true, s));
      FS_TRY(mult.reserve((size_t)mult_bytes));
      FS_TRY(counts.reserve(rows * a.Bp));
      FS_TRY(order.reserve(2 * (size_t)n_units));
      a.mult = mult.p;
      a.counts = counts.p;
    }
    FS_TRY(clk.mark(0, s));
    if (some) inc.incidence(d_rows, a, s);
    FS_TRY(clk.mark(1, s));
    hipLaunchKernelGGL(k_int_totals, dim3(a.B), blk, 0, s, a);
    if (some)
      hipLaunchKernelGGL(k_int_mult, dim3(blocks_of((uint64_t)a.Bp * (a.Wp / 4), kRunBlock)), blk,
                         0, s, a);
    FS_TRY(clk.mark(2, s));
    if (some) {
      if (mfma) {
        // few tiles: the words k are shared out (inc_ksplit)
        const uint32_t gy = (a.Bp / 16 + 4 * kRT - 1) / (4 * kRT);
        a.ksplit = inc_ksplit("FS_INTERVALS_KSPLIT", (uint64_t)a.m.n_tiles * gy, a.m.nk);
        if (a.ksplit > 1)
          FS_HIP(hipMemsetAsync(counts.p, 0, rows * a.Bp * sizeof(uint32_t), s));
        hipLaunchKernelGGL(k_int_product, dim3(a.m.n_tiles, gy, a.ksplit), dim3(kProd), 0, s, a);
      } else
        hipLaunchKernelGGL(k_int_plain, dim3((uint32_t)rows, blocks_of(a.Bp, kRunBlock)), blk, 0,
                           s, a);
    }
    FS_TRY(clk.mark(3, s));
    if (some) {
      hipLaunchKernelGGL(k_int_stats, dim3(n_units), dim3(kStat), 0, s, a);
      hipLaunchKernelGGL(k_int_quoted, dim3(blocks_of(n_units, kRunBlock), (a.B + 63) / 64), blk,
                         0, s, a);
    }
    FS_TRY(clk.mark(4, s));
    FS_HIP(hipGetLastError());
    if (some) {
      // the observed order: works descending, then the unit; rank = 1 + the units with more
      std::vector<uint32_t> works(n_units), at(n_units), rn(2 * (size_t)n_units);
      FS_HIP(hipMemcpyAsync(works.data(), a.m.covered, (size_t)n_units * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
      for (uint32_t u = 0; u < n_units; ++u) at[u] = u;
      std::stable_sort(at.begin(), at.end(),
                       [&works](uint32_t x, uint32_t y) { return works[x] > works[y]; });
      uint32_t rank = 1;
      for (uint32_t i = 0; i < n_units; ++i) {
        if (i && works[at[i]] != works[at[i - 1]]) rank = i + 1;
        rn[at[i]] = rank;
        rn[(size_t)n_units + at[i]] = i + 1 < n_units ? at[i + 1] : FS_NONE;
      }
      FS_TRY(order.upload(rn.data(), rn.size(), s));
      a.rank = order.p;
      a.next = order.p + n_units;
      hipLaunchKernelGGL(k_int_units, dim3(blocks_of(n_units, kRunBlock / 64)), blk, 0, s, a);
      FS_TRY(clk.mark(5, s));
      hipLaunchKernelGGL(k_int_reps, dim3(blocks_of(a.B, kRunBlock)), blk, 0, s, a);
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));                     // (rn is read until here)
    } else {
      if (n_units)
        hipLaunchKernelGGL(k_int_none, dim3(blocks_of(n_units, kRunBlock)), blk, 0, s, a);
      FS_TRY(clk.mark(5, s));
      hipLaunchKernelGGL(k_int_reps, dim3(blocks_of(a.B, kRunBlock)), blk, 0, s, a);
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));
    }
    for (int k = 0; k < 5; ++k) t_ms[k] = clk.elapsed(k, k + 1);
    t_ms[5] = t_ms[0] + t_ms[1] + t_ms[2] + t_ms[3] + t_ms[4];
    return FS_OK;
  }
};

// the rules both entry points share
int int_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, const void* unit_of,
              uint32_t n_units, uint32_t min_words, uint32_t replicates, uint32_t level,
              const void* units, const void* reps) {
  if (!reps || (n_units && !units) || (n_rows && n_units && n_script && !unit_of)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (replicates == 0 || replicates > FS_INTERVALS_MAX_REPLICATES) {
    fs_set_error("replicates %u: from 1 to %u", replicates, FS_INTERVALS_MAX_REPLICATES);
    return FS_E_INVALID;
  }
  if (level < 50 || level > 99) {
    fs_set_error("level %u: a whole percentage from 50 to 99", level);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("intervals", n_rows, n_script));
  if (n_works > FS_INTERVALS_MAX_WORKS) {
    fs_set_error("n_works %u: intervals take up to %u", n_works, FS_INTERVALS_MAX_WORKS);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_intervals(int device, const uint32_t* work, const uint32_t* fan_ix,
                            const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                            uint32_t n_script, const uint32_t* unit_of, uint32_t n_units,
                            uint32_t min_words, uint32_t max_gap, uint32_t replicates,
                            uint64_t seed, uint32_t level, fs_interval_unit* units,
                            fs_interval_replicate* reps) {
  FS_TRY(int_check(n_rows, n_works, n_script, unit_of, n_units, min_words, replicates, level,
                   units, reps));
  if (n_rows && (!work || !fan_ix || !orig_ix)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<uint32_t> d_unit_of;
  DBuf<fs_interval_unit> d_units;
  DBuf<fs_interval_replicate> d_reps;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_unit_of.upload(unit_of, n && n_units ? n_script : 0, nullptr));
  FS_TRY(d_units.reserve(n_units));
  FS_TRY(d_reps.reserve(replicates));
  IntJob job;
  FS_TRY(job.run(rows.p, n, n_works, n_script, d_unit_of.p, n_units, min_words, max_gap, replicates,
                 seed, level, d_units.p, d_reps.p, nullptr));
  if (n_units) FS_TRY(copy_out(units, d_units, n_units));
  FS_TRY(copy_out(reps, d_reps, replicates));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_intervals_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                 uint32_t n_works, const uint32_t* d_unit_of, uint32_t n_units,
                                 uint32_t min_words, uint32_t max_gap, uint32_t replicates,
                                 uint64_t seed, uint32_t level, fs_interval_unit* d_units,
                                 fs_interval_replicate* d_reps) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: intervals take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(int_check(n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units, min_words,
                   replicates, level, d_units, d_reps));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_unit_of & 3) ||
      ((uintptr_t)d_units & 15) || ((uintptr_t)d_reps & 15)) {
    fs_set_error("d_rows, d_units and d_reps must be 16-byte aligned device pointers, "
                 "d_unit_of 4-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  IntJob job;
  return job.run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, d_unit_of, n_units,
                 min_words, max_gap, replicates, seed, level, d_units, d_reps, ix->stream);
}

extern "C" int fs_intervals_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
