// fs_prims.h -- what the command units (fs_passages.hip ... fs_companions.hip, fs_matches.hip,
// fs_tiles.h) share: wave reductions and scans, workgroup scans and ranks, the one-workgroup
// chunked scan, the view of the match records, and the host's pass clock, environment bounds
// and record limits.  A command unit takes its scans, ranks and wave reductions from here and
// reads its records through RowsSrc: fs_row records in device memory, whether a search left
// them there or fs_host_rows (fs_internal.h) packed them from the columns a caller passed.
// Everything is integer arithmetic: no schedule changes a result.  (The search path keeps its
// own DPP versions in fs_device.h.)
#pragma once
#include "fs_internal.h"

#include <stdlib.h>

// ---- a wave of 64 lanes (T: uint32_t or uint64_t) ----

template <class T>
__device__ inline T wave_sum(T v) {
  for (uint32_t d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <class T>
__device__ inline T wave_max(T v) {
  for (uint32_t d = 32; d; d >>= 1) {
    const T o = __shfl_xor(v, d);
    if (o > v) v = o;
  }
  return v;
}

// the same inside every aligned segment of `width` lanes (a power of two up to 64, the same in
// every lane of the wave)
template <class T>
__device__ inline T seg_sum(T v, uint32_t width) {
  for (uint32_t d = width >> 1; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <class T>
__device__ inline T seg_max(T v, uint32_t width) {
  for (uint32_t d = width >> 1; d; d >>= 1) {
    const T o = __shfl_xor(v, d);
    if (o > v) v = o;
  }
  return v;
}

// inclusive scan in lane order
template <class T>
__device__ inline T wave_scan(T v) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(v, d);
    if (lane >= d) v += y;
  }
  return v;
}

__device__ inline uint32_t lane_u32(uint32_t v, uint32_t s) {      // s wave-uniform
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)s);
}

// the first active lane's value in every lane
template <class T>
__device__ inline T wave_first(T v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  if constexpr (sizeof(T) == 4) {
    return lo;
  } else {
    const uint32_t up = (uint32_t)((uint64_t)v >> 32);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)up);
    return (T)((uint64_t)hi << 32 | lo);
  }
}

// values written and read back inside one kernel, by other lanes of the wave too: past the
// CU's vector cache
__device__ inline uint32_t ld_agent(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline void st_agent(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- a workgroup of kThreads threads; s_w is kThreads / 64 words of LDS, free on return ----

// exclusive scan of x in thread order; *total = the workgroup's sum.  s_w is still being read
// on return: a __syncthreads() comes before its next use
template <uint32_t kThreads, class T>
__device__ inline T block_scan_open(T x, T* s_w, T* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan(x);
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  T pre = 0, tot = 0;
  for (uint32_t w = 0; w < kThreads / 64; ++w) {       // one chain of sums: pre is tot on the way
    if (w == wave) pre = tot;
    tot += s_w[w];
  }
  *total = tot;
  return pre + inc - x;
}

// the same, s_w free on return
template <uint32_t kThreads, class T>
__device__ inline T block_scan(T x, T* s_w, T* total) {
  const T pre = block_scan_open<kThreads>(x, s_w, total);
  __syncthreads();                         // s_w read by every wave
  return pre;
}

// rank of a flagged thread among the flagged threads of its workgroup, and their number
template <uint32_t kThreads>
__device__ inline void block_rank(bool flag, uint32_t* s_w, uint32_t* rank, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t b = __ballot(flag);
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t pre = (uint32_t)__popcll(b & ((1ull << lane) - 1)), tot = 0;
  for (uint32_t w = 0; w < kThreads / 64; ++w) {
    if (w < wave) pre += s_w[w];
    tot += s_w[w];
  }
  *rank = pre;
  *total = tot;
  __syncthreads();                         // s_w may be used again
}

// ---- the scan of a whole array by one workgroup of kScanBlock threads ----

constexpr uint32_t kScanBlock = 1024;

// Items 0 .. n in chunks of kScanBlock * kItems in turn, kItems adjacent ones per thread:
// store(j, the sum of the items in front of j, item j) for every j < n; returns the sum of all.
// An item is a V = load(j) and is summed as a V inside its chunk; the carry from chunk to
// chunk is a T in a register.  s_w: kScanBlock / 64 words of LDS.
template <uint32_t kItems, class V, class T, class Load, class Store>
__device__ inline T scan_chunks(uint64_t n, Load load, Store store, V* s_w) {
  T carry = 0;
  for (uint64_t c = 0; c < n; c += (uint64_t)kScanBlock * kItems) {
    const uint64_t j0 = c + (uint64_t)threadIdx.x * kItems;
    V x[kItems], mine = 0, total;
#pragma unroll
    for (uint32_t t = 0; t < kItems; ++t) {
      x[t] = j0 + t < n ? load(j0 + t) : (V)0;
      mine += x[t];
    }
    T at = carry + block_scan_open<kScanBlock>(mine, s_w, &total);
#pragma unroll
    for (uint32_t t = 0; t < kItems; ++t) {
      if (j0 + t < n) store(j0 + t, at, x[t]);
      at += x[t];
    }
    carry += total;
    __syncthreads();                       // behind the stores: s_w read by every wave
  }
  return carry;
}

// The body of a unit's k_*_scan kernel: exclusive scan of in[j * kStride], j < n, into out[j]
// (which may be in), *total = the sum.
template <class V, class T, uint32_t kStride = 1, class In, class Out>
__device__ inline void scan_array(const In* in, uint64_t n, Out* out, T* total) {
  __shared__ V s_w[kScanBlock / 64];
  const T sum = scan_chunks<1, V, T>(
      n, [in](uint64_t j) { return (V)in[j * kStride]; },
      [out](uint64_t j, T pre, V) { out[j] = (Out)pre; }, s_w);
  if (threadIdx.x == 0) *total = sum;
}

// ---- the match records ----

// the key half {work, fan_ix, orig_ix, lev} and the value half {dist, comb}, one 16-byte load
// each (rows are 16-byte aligned, 32 bytes apart)
struct RowsSrc {
  const fs_row* rows;
  __device__ uint4 key(uint64_t i) const { return reinterpret_cast<const uint4*>(rows + i)[0]; }
  __device__ double2 val(uint64_t i) const { return reinterpret_cast<const double2*>(rows + i)[1]; }
  __device__ double comb(uint64_t i) const { return rows[i].comb; }
};

// ---- host (internal linkage: the library exports none of these) ----
// An unnamed namespace in a header, on purpose: every unit that includes it already keeps its
// code in one, and gets its own copy of these few lines.

namespace {

inline uint32_t blocks_of(uint64_t count, uint32_t block) {
  return (uint32_t)((count + block - 1) / block);
}

// an unsigned bound from the environment (diagnostics, read on each call): dflt when unset,
// at most `most`
inline uint32_t env_u32(const char* name, uint32_t dflt, uint32_t most) {
  const char* e = getenv(name);
  if (!e || !*e) return dflt;
  const unsigned long long v = strtoull(e, nullptr, 10);
  return v > most ? most : (uint32_t)v;
}

// HIP events around the passes of one call
template <int kMarks>
struct Clock {
  hipEvent_t ev[kMarks] = {};
  bool set[kMarks] = {};
  ~Clock() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int mark(int k, hipStream_t s) {
    if (!ev[k]) FS_HIP(hipEventCreate(&ev[k]));
    FS_HIP(hipEventRecord(ev[k], s));
    set[k] = true;
    return FS_OK;
  }
  double elapsed(int from, int to) {       // 0 unless both were marked
    float ms = 0.f;
    if (!set[from] || !set[to]) return 0.0;
    return hipEventElapsedTime(&ms, ev[from], ev[to]) == hipSuccess ? (double)ms : 0.0;
  }
};

// ---- what the entry points share ----

// the first n records of a device buffer to the host, when the device is done with them
template <class T>
inline int copy_out(T* host, const DBuf<T>& d, size_t n) {
  FS_HIP(hipMemcpy(host, d.p, n * sizeof(T), hipMemcpyDeviceToHost));
  return FS_OK;
}

// fs_X_times: the n stage times the last call of a unit left in t_ms
inline int times_out(double* ms, const double* t_ms, int n) {
  if (!ms) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  for (int k = 0; k < n; ++k) ms[k] = t_ms[k];
  return FS_OK;
}

// the two bounds most units put on their records: fewer than 2^32 of them, and a script of at
// most FS_WORKS_MAX_SCRIPT words
inline int record_limits(const char* what, uint64_t n_rows, uint32_t n_script) {
  if (n_rows >= (1ull << 32)) {
    fs_set_error("%llu records: %s take fewer than 2^32", (unsigned long long)n_rows, what);
    return FS_E_UNSUPPORTED;
  }
  if (n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("n_script %u: %s take up to %u", n_script, what, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  return FS_OK;
}

}  // namespace
