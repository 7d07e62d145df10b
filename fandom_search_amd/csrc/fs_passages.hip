// fs_passages.hip -- `ao3.py passages`: match records sorted by (work, fan_ix) joined into
// runs (record s continues record r before it when both are of one work and the fan and the
// script index each step 1..1+G ahead), runs of at least M records kept, with their sums and
// maxima (fs_passages, fs_passages_rows in include/fandom_search.h).
//
// Reduce-then-scan over separate launches; no workgroup waits on another:
//   k_pass_heads   head flag per record (64-bit ballot words), sortedness, heads per tile
//   k_pass_scan    one workgroup: exclusive scan of the per-tile counts, total
//   k_pass_place   head positions, compacted
//   k_pass_kept    one lane per run: kept flag (length >= M) words, kept runs per tile
//   k_pass_scan    again, over those counts
//   k_pass_reduce  one lane per run: sums and maxima of a kept run, written to its slot
// Sums are walked in record order by one lane (or, for a long run, by the whole wave in
// lock-step, every lane adding the same values in the same order).
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kItems = 16;
constexpr uint32_t kTile = kBlock * kItems;     // records (runs) per workgroup: 64 ballot words
constexpr uint32_t kLong = 256;                 // runs of this many records are walked by a wave

// s continues r: same work, 1 <= fan step <= 1 + G, 1 <= script step <= 1 + G (signed)
__device__ inline bool joins(uint4 r, uint4 s, int64_t g1) {
  const int64_t df = (int64_t)s.y - (int64_t)r.y;
  const int64_t dr = (int64_t)s.z - (int64_t)r.z;
  return s.x == r.x && df >= 1 && df <= g1 && dr >= 1 && dr <= g1;
}

// per-tile total of the waves' ballot counts into cnt[blockIdx.x]
__device__ inline void tile_count(uint32_t wave_count, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t s_c[kBlock / 64];
  if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = wave_count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < kBlock / 64; ++w) t += s_c[w];
    cnt[blockIdx.x] = t;
  }
}

// s_pre[w] = flags of this tile in front of its ballot word w (words are in record order:
// word k * 4 + wave holds item k of wave `wave`)
__device__ inline void tile_prefix(const uint64_t* __restrict__ mask, uint64_t n_words,
                                   uint32_t* s_pre) {
  if (threadIdx.x < 64) {
    const uint32_t lane = threadIdx.x;
    const uint64_t w = (uint64_t)blockIdx.x * (kTile / 64) + lane;
    const uint32_t c = w < n_words ? (uint32_t)__popcll(mask[w]) : 0u;
    s_pre[lane] = wave_scan(c) - c;
  }
  __syncthreads();
}

// the three key columns of records that never were fs_row records (fs_readings.hip)
struct KeyCols {
  const uint32_t* work;
  const uint32_t* fan;
  const uint32_t* orig;
  __device__ uint4 key(uint64_t i) const { return make_uint4(work[i], fan[i], orig[i], 0); }
};

// Src: RowsSrc or KeyCols (the one kernel compiled for both)
template <class Src>
__global__ __launch_bounds__(kBlock) void k_pass_heads(Src src, uint32_t n, int64_t g1,
                                                       uint64_t* __restrict__ mask,
                                                       uint32_t* __restrict__ cnt,
                                                       uint32_t* __restrict__ status) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  uint32_t heads = 0;
  bool bad = false;
  for (uint32_t k = 0; k < kItems; ++k) {
    const uint64_t i = base + k * kBlock + threadIdx.x;
    bool head = false;
    if (i < n) {
      const uint4 s = src.key(i);
      head = true;
      if (i > 0) {
        const uint4 r = src.key(i - 1);
        bad |= s.x < r.x || (s.x == r.x && s.y < r.y);
        head = !joins(r, s, g1);
      }
    }
    const uint64_t b = __ballot(head);
    if (lane == 0 && i < n) mask[i >> 6] = b;
    heads += (uint32_t)__popcll(b);
  }
  if (__ballot(bad) && lane == 0) atomicOr(&status[1], 1u);
  tile_count(heads, cnt);
}

// exclusive scan of v[0..nb) in place, *total = sum (one workgroup, chunks of 1024 in turn)
__global__ __launch_bounds__(kScanBlock) void k_pass_scan(uint32_t* v, uint32_t nb,
                                                          uint32_t* __restrict__ total) {
  scan_array<uint32_t, uint32_t>(v, nb, v, total);
}

// heads[k] = index of the first record of run k; heads[n_runs] = n
__global__ __launch_bounds__(kBlock) void k_pass_place(const uint64_t* __restrict__ mask,
                                                       const uint32_t* __restrict__ off, uint32_t n,
                                                       const uint32_t* __restrict__ status,
                                                       uint32_t* __restrict__ heads) {
  __shared__ uint32_t s_pre[64];
  tile_prefix(mask, ((uint64_t)n + 63) >> 6, s_pre);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  const uint32_t o = off[blockIdx.x];
  for (uint32_t k = 0; k < kItems; ++k) {
    const uint64_t i = base + k * kBlock + threadIdx.x;
    if (i >= n) break;
    const uint64_t m = mask[i >> 6];
    if ((m >> lane) & 1)
      heads[o + s_pre[k * (kBlock / 64) + wave] + (uint32_t)__popcll(m & ((1ull << lane) - 1))] =
          (uint32_t)i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) heads[status[0]] = n;
}

// kept flag per run (at least min_words records), ballot words and per-tile counts
__global__ __launch_bounds__(kBlock) void k_pass_kept(const uint32_t* __restrict__ heads,
                                                      uint32_t n_runs, uint32_t min_words,
                                                      uint64_t* __restrict__ mask,
                                                      uint32_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  uint32_t kept = 0;
  for (uint32_t k = 0; k < kItems; ++k) {
    const uint64_t r = base + k * kBlock + threadIdx.x;
    const bool keep = r < n_runs && heads[r + 1] - heads[r] >= min_words;
    const uint64_t b = __ballot(keep);
    if (lane == 0 && r < n_runs) mask[r >> 6] = b;
    kept += (uint32_t)__popcll(b);
  }
  tile_count(kept, cnt);
}

struct Acc {
  uint32_t n_exact;
  double dist_sum, dist_max, comb_sum, comb_max;
};

__device__ inline Acc acc_init() {
  const double nan = __builtin_nan("");
  return Acc{0u, 0.0, nan, 0.0, nan};
}

// maximum over non-NaN values, the earlier one kept on a tie
__device__ inline void max_upd(double& m, double v) {
  if (!(v <= m) && !isnan(v)) m = v;
}

__device__ inline void acc_add(Acc& a, double d, double c) {
  a.dist_sum += d;
  a.comb_sum += c;
  a.n_exact += c <= 0.0 ? 1u : 0u;
  max_upd(a.dist_max, d);
  max_upd(a.comb_max, c);
}

// lane t's value, as a wave-uniform scalar (t uniform)
__device__ inline double lane_value(double v, uint32_t t) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), (int)t);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), (int)t);
  return __hiloint2double(hi, lo);
}

// records [b, e) by one lane, eight loads in flight ahead of their adds
__device__ inline Acc lane_walk(const RowsSrc& src, uint64_t b, uint64_t e) {
  Acc a = acc_init();
  uint64_t i = b;
  for (; i + 8 <= e; i += 8) {
    double2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = src.val(i + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc_add(a, v[k].x, v[k].y);
  }
  for (; i < e; ++i) {
    const double2 v = src.val(i);
    acc_add(a, v.x, v.y);
  }
  return a;
}

// records [b, e) (wave-uniform bounds) by the whole wave: 64 records per load, the next 64
// requested before the current ones are added; every lane adds all of them in record order
__device__ inline Acc wave_walk(const RowsSrc& src, uint64_t b, uint64_t e, uint32_t lane) {
  Acc a = acc_init();
  double2 cur = b + lane < e ? src.val(b + lane) : make_double2(0.0, 0.0);
  for (uint64_t c = b; c < e; c += 64) {
    const uint64_t j = c + 64 + lane;
    const double2 nxt = j < e ? src.val(j) : make_double2(0.0, 0.0);
    const uint32_t cnt = e - c < 64 ? (uint32_t)(e - c) : 64u;
    for (uint32_t t = 0; t < cnt; ++t) acc_add(a, lane_value(cur.x, t), lane_value(cur.y, t));
    cur = nxt;
  }
  return a;
}

__global__ __launch_bounds__(kBlock) void k_pass_reduce(RowsSrc src,
                                                        const uint32_t* __restrict__ heads,
                                                        uint32_t n_runs,
                                                        const uint64_t* __restrict__ mask,
                                                        const uint32_t* __restrict__ off,
                                                        fs_passage* __restrict__ out) {
  __shared__ uint32_t s_pre[64];
  tile_prefix(mask, ((uint64_t)n_runs + 63) >> 6, s_pre);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  const uint32_t o = off[blockIdx.x];
  for (uint32_t k = 0; k < kItems; ++k) {
    const uint64_t r = base + k * kBlock + threadIdx.x;
    bool kept = false;
    uint32_t b = 0, e = 0, pos = 0;
    if (r < n_runs) {
      const uint64_t m = mask[r >> 6];
      kept = (m >> lane) & 1;
      if (kept) {
        b = heads[r];
        e = heads[r + 1];
        pos = o + s_pre[k * (kBlock / 64) + wave] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
      }
    }
    const bool is_long = kept && e - b >= kLong;
    Acc a = acc_init();
    for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
      const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
      const uint32_t bj = (uint32_t)__builtin_amdgcn_readlane((int)b, j);
      const uint32_t ej = (uint32_t)__builtin_amdgcn_readlane((int)e, j);
      const Acc w = wave_walk(src, bj, ej, lane);
      if ((int)lane == j) a = w;
    }
    if (kept && !is_long) a = lane_walk(src, b, e);
    if (kept) {
      fs_passage p;
      p.first = b;
      p.n_words = e - b;
      p.n_exact = a.n_exact;
      p.dist_sum = a.dist_sum;
      p.dist_max = a.dist_max;
      p.comb_sum = a.comb_sum;
      p.comb_max = a.comb_max;
      out[pos] = p;
    }
  }
}

// device scratch of one call
struct PassWork {
  DBuf<uint64_t> mask, mask2;
  DBuf<uint32_t> cnt, cnt2, heads, status;
  uint32_t n = 0, n_runs = 0, n_kept = 0;
};

uint32_t tiles(uint64_t count) { return (uint32_t)((count + kTile - 1) / kTile); }

// runs and kept runs: w.n_runs, w.n_kept; FS_E_INVALID on records out of (work, fan_ix) order
template <class Src>
int pass_count(const Src& src, uint32_t n, uint32_t min_words, uint32_t max_gap, PassWork& w,
               hipStream_t s) {
  w.n = n;
  const uint32_t nb = tiles(n);
  FS_TRY(w.mask.reserve(((uint64_t)n + 63) >> 6));
  FS_TRY(w.cnt.reserve(nb));
  FS_TRY(w.status.reserve(4));
  FS_HIP(hipMemsetAsync(w.status.p, 0, 4 * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_pass_heads<Src>, dim3(nb), dim3(kBlock), 0, s, src, n,
                     (int64_t)max_gap + 1, w.mask.p, w.cnt.p, w.status.p);
  hipLaunchKernelGGL(k_pass_scan, dim3(1), dim3(kScanBlock), 0, s, w.cnt.p, nb, w.status.p);
  FS_HIP(hipGetLastError());
  uint32_t st[2];
  FS_HIP(hipMemcpyAsync(st, w.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[1]) {
    fs_set_error("records are not sorted by (work, fan_ix)");
    return FS_E_INVALID;
  }
  w.n_runs = st[0];
  const uint32_t nr = tiles(w.n_runs);
  FS_TRY(w.heads.reserve((uint64_t)w.n_runs + 1));
  FS_TRY(w.mask2.reserve(((uint64_t)w.n_runs + 63) >> 6));
  FS_TRY(w.cnt2.reserve(nr));
  hipLaunchKernelGGL(k_pass_place, dim3(nb), dim3(kBlock), 0, s, w.mask.p, w.cnt.p, n, w.status.p,
                     w.heads.p);
  hipLaunchKernelGGL(k_pass_kept, dim3(nr), dim3(kBlock), 0, s, w.heads.p, w.n_runs, min_words,
                     w.mask2.p, w.cnt2.p);
  hipLaunchKernelGGL(k_pass_scan, dim3(1), dim3(kScanBlock), 0, s, w.cnt2.p, nr, w.status.p + 2);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(&w.n_kept, w.status.p + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  return FS_OK;
}

// Both entry points behind their checks: the kept passages of n records on `s`, into `out`
// on the host (by way of a device buffer of the call's own) or into d_out on the device.
int pass_run(const fs_row* d_rows, uint32_t n, uint32_t min_words, uint32_t max_gap,
             fs_passage* out, fs_passage* d_out, uint64_t cap, uint64_t* n_out, hipStream_t s) {
  PassWork w;
  FS_TRY(pass_count(RowsSrc{d_rows}, n, min_words, max_gap, w, s));
  *n_out = w.n_kept;
  if (w.n_kept > cap) return FS_E_CAPACITY;
  DBuf<fs_passage> d_own;
  if (out) {
    FS_TRY(d_own.reserve(w.n_kept));
    d_out = d_own.p;
  }
  if (w.n_kept) {
    hipLaunchKernelGGL(k_pass_reduce, dim3(tiles(w.n_runs)), dim3(kBlock), 0, s, RowsSrc{d_rows},
                       w.heads.p, w.n_runs, w.mask2.p, w.cnt2.p, d_out);
    FS_HIP(hipGetLastError());
    if (out) FS_TRY(copy_out(out, d_own, w.n_kept));
  }
  return FS_OK;
}

// the rules both entry points share; *done when nothing is left to do
int pass_check(uint64_t n_rows, uint32_t min_words, const void* out, uint64_t cap,
               uint64_t* n_out, bool* done) {
  *done = false;
  if (!n_out || (cap && !out)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: passages take fewer than 2^32", (unsigned long long)n_rows);
    return FS_E_UNSUPPORTED;
  }
  *n_out = 0;
  *done = n_rows == 0;
  return FS_OK;
}

}  // namespace

// The runs of records sorted by (work, fan_ix), exactly as the passages join them, for the
// other command units (declared in fs_internal.h).
struct fs_runs {
  PassWork w;
};

namespace {

template <class Src>
int runs_find(const Src& src, uint32_t n, uint32_t min_words, uint32_t max_gap, hipStream_t s,
              fs_runs** runs, const uint32_t** d_heads, uint32_t* n_runs) {
  fs_runs* r = new fs_runs;
  const int rc = pass_count(src, n, min_words, max_gap, r->w, s);
  if (rc != FS_OK) {
    delete r;
    return rc;
  }
  *runs = r;
  *d_heads = r->w.heads.p;
  *n_runs = r->w.n_runs;
  return FS_OK;
}

// a record per thread; the doubles travel as their bits
__global__ __launch_bounds__(kBlock) void k_rows_pack(const uint32_t* __restrict__ work,
                                                      const uint32_t* __restrict__ fan,
                                                      const uint32_t* __restrict__ orig,
                                                      const uint2* __restrict__ dist,
                                                      const uint2* __restrict__ comb,
                                                      const uint8_t* __restrict__ exact, uint32_t n,
                                                      fs_row* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint2 d = dist ? dist[i] : make_uint2(0u, 0u);
  uint2 c = comb ? comb[i] : make_uint2(0u, 0u);
  if (exact) c.y = exact[i] ? 0u : 0x3FF00000u;              // 0.0 : 1.0
  uint4* o = reinterpret_cast<uint4*>(rows + i);
  o[0] = make_uint4(work[i], fan[i], orig[i], 0u);
  o[1] = make_uint4(d.x, d.y, c.x, c.y);
}

}  // namespace

int fs_runs_find(const fs_row* d_rows, uint32_t n, uint32_t min_words, uint32_t max_gap,
                 hipStream_t s, fs_runs** runs, const uint32_t** d_heads, uint32_t* n_runs) {
  return runs_find(RowsSrc{d_rows}, n, min_words, max_gap, s, runs, d_heads, n_runs);
}

int fs_runs_find_cols(const uint32_t* d_work, const uint32_t* d_fan, const uint32_t* d_orig,
                      uint32_t n, uint32_t min_words, uint32_t max_gap, hipStream_t s,
                      fs_runs** runs, const uint32_t** d_heads, uint32_t* n_runs) {
  return runs_find(KeyCols{d_work, d_fan, d_orig}, n, min_words, max_gap, s, runs, d_heads,
                   n_runs);
}

void fs_runs_free(fs_runs* r) { delete r; }

int fs_host_rows(DBuf<fs_row>& rows, const uint32_t* work, const uint32_t* fan,
                 const uint32_t* orig, size_t n, const double* dist, const double* comb,
                 const uint8_t* exact) {
  // one staging buffer: the 8-byte columns first, then the 4-byte ones, then the flags
  const size_t nd = dist ? n : 0, nc = comb ? n : 0, ne = exact ? n : 0;
  DBuf<unsigned char> stage;
  FS_TRY(stage.reserve((nd + nc) * sizeof(double) + 3 * n * sizeof(uint32_t) + ne));
  double* d_dist = reinterpret_cast<double*>(stage.p);
  double* d_comb = d_dist + nd;
  uint32_t* d_work = reinterpret_cast<uint32_t*>(d_comb + nc);
  uint32_t *d_fan = d_work + n, *d_orig = d_fan + n;
  uint8_t* d_exact = reinterpret_cast<uint8_t*>(d_orig + n);
  const auto up = [](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, nullptr) : hipSuccess;
  };
  FS_HIP(up(d_work, work, n * sizeof(uint32_t)));
  FS_HIP(up(d_fan, fan, n * sizeof(uint32_t)));
  FS_HIP(up(d_orig, orig, n * sizeof(uint32_t)));
  FS_HIP(up(d_dist, dist, nd * sizeof(double)));
  FS_HIP(up(d_comb, comb, nc * sizeof(double)));
  FS_HIP(up(d_exact, exact, ne));
  FS_TRY(rows.reserve(n));
  if (n) {
    hipLaunchKernelGGL(k_rows_pack, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, nullptr, d_work,
                       d_fan, d_orig, nd ? reinterpret_cast<const uint2*>(d_dist) : nullptr,
                       nc ? reinterpret_cast<const uint2*>(d_comb) : nullptr,
                       ne ? d_exact : nullptr, (uint32_t)n, rows.p);
    FS_HIP(hipGetLastError());
  }
  return FS_OK;                     // `stage` is freed here, behind the kernel that reads it
}

extern "C" int fs_passages(int device, const uint32_t* work, const uint32_t* fan_ix,
                           const uint32_t* orig_ix, const double* dist, const double* comb,
                           uint64_t n_rows, uint32_t min_words, uint32_t max_gap, fs_passage* out,
                           uint64_t cap, uint64_t* n_out) {
  bool done = false;
  FS_TRY(pass_check(n_rows, min_words, out, cap, n_out, &done));
  if (done) return FS_OK;
  if (!work || !fan_ix || !orig_ix || !dist || !comb) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  DBuf<fs_row> rows;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n_rows, dist, comb));
  FS_TRY(pass_run(rows.p, (uint32_t)n_rows, min_words, max_gap, out, nullptr, cap, n_out, nullptr));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_passages_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                uint32_t min_words, uint32_t max_gap, fs_passage* d_out,
                                uint64_t cap, uint64_t* n_out) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  bool done = false;
  FS_TRY(pass_check(n_rows, min_words, d_out, cap, n_out, &done));
  if (done) return FS_OK;
  if (!d_rows || ((uintptr_t)d_rows & 15) || ((uintptr_t)d_out & 7)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_out 8-byte aligned");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  FS_TRY(pass_run(d_rows, (uint32_t)n_rows, min_words, max_gap, nullptr, d_out, cap, n_out,
                  ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  return FS_OK;
}
