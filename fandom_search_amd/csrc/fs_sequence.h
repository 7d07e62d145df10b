// fs_sequence.h -- a work's unit-bearing passage sequence, shared by fs_transitions.hip and
// fs_routes.hip: the checks of the records and of the unit map, the run heads as fs_passages
// joins them, and the kept runs that start in a unit listed in record order as columns (work,
// first and last fan word, first and last script word, unit).  What each unit makes of the
// sequence (steps between neighbours; collapsed routes) is its own.
//
// Separate launches; no workgroup waits on another:
//   k_tr_check     one lane per record: work < n_works, orig_ix < n_script
//   k_tr_units_ok  one lane per script word: a unit number that is neither < n_units nor none
//   (fs_runs_find) the run heads
//   k_tr_seq       one lane per run: kept runs that start in a unit counted per workgroup, then
//                  (after k_tr_scan) placed in record order
#pragma once
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kSeqBlock = 256;

// status words
enum { kStBadRecord = 0, kStBadUnit = 1, kStSeq = 2, kStWords = 4 };

struct SeqArgs {
  const uint32_t* heads;         // [n_runs + 1]
  const uint32_t* unit_of;       // [n_script]
  uint32_t n, n_runs, n_works, n_script, n_units, n_seq;
  uint32_t min_words;
  uint32_t* cnt;                 // [workgroups of runs] listed runs, then their exclusive scan
  uint32_t* work;                // [n_seq] each: the sequence elements in record order
  uint32_t* ff;
  uint32_t* fl;
  uint32_t* of;
  uint32_t* ol;
  uint32_t* unit;
  uint32_t* status;
};

__global__ __launch_bounds__(kSeqBlock) void k_tr_check(RowsSrc src, SeqArgs a) {
  const uint32_t i = blockIdx.x * kSeqBlock + threadIdx.x;
  bool bad = false;
  if (i < a.n) {
    const uint4 k = src.key(i);
    bad = k.x >= a.n_works || k.z >= a.n_script;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStBadRecord], 1u);
}

__global__ __launch_bounds__(kSeqBlock) void k_tr_units_ok(SeqArgs a) {
  const uint32_t o = blockIdx.x * kSeqBlock + threadIdx.x;
  bool bad = false;
  if (o < a.n_script) {
    const uint32_t u = a.unit_of[o];
    bad = u != FS_NONE && u >= a.n_units;
  }
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStBadUnit], 1u);
}

__global__ __launch_bounds__(kScanBlock) void k_tr_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t n, unsigned long long* total32,
                                                        uint32_t* total) {
  __shared__ unsigned long long s_total;
  scan_array<uint32_t, unsigned long long>(in, n, out, &s_total);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (total32) *total32 = s_total;
    if (total) *total = (uint32_t)s_total;
  }
}

// kPlace false: the kept runs with a unit of this workgroup's 256 runs into cnt; true: those
// runs to their places, cnt holding the scan.  (Every orig_ix is below n_script here:
// k_tr_check found nothing.)
template <bool kPlace>
__global__ __launch_bounds__(kSeqBlock) void k_tr_seq(RowsSrc src, SeqArgs a) {
  __shared__ uint32_t s_w[kSeqBlock / 64];
  const uint32_t r = blockIdx.x * kSeqBlock + threadIdx.x;
  uint32_t b = 0, e = 0, u = FS_NONE;
  uint4 x = make_uint4(0u, 0u, 0u, 0u);
  if (r < a.n_runs) {
    b = a.heads[r];
    e = a.heads[r + 1];
    if (e - b >= a.min_words) {
      x = src.key(b);
      u = a.unit_of[x.z];
    }
  }
  const bool keep = u != FS_NONE;
  uint32_t rank, total;
  block_rank<kSeqBlock>(keep, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = total;
  } else if (keep) {
    const uint32_t p = a.cnt[blockIdx.x] + rank;
    const uint4 y = src.key(e - 1);
    a.work[p] = x.x;
    a.ff[p] = x.y;
    a.fl[p] = y.y;
    a.of[p] = x.z;
    a.ol[p] = y.z;
    a.unit[p] = u;
  }
}

// the buffers behind a SeqArgs and the launches that fill them
struct SeqJob {
  DBuf<uint32_t> status, cnt, seq;
  fs_runs* runs = nullptr;
  ~SeqJob() { if (runs) fs_runs_free(runs); }

  // a.n, n_works, n_script, unit_of, n_units and min_words set by the caller (n and n_units not
  // 0): the checks, then a.n_seq elements in a.work .. a.unit (all on `s`, finished on return)
  int list(const fs_row* d_rows, SeqArgs& a, uint32_t max_gap, hipStream_t s) {
    const RowsSrc src{d_rows};
    if (!a.n_works || !a.n_script) {
      fs_set_error("a work >= n_works or an orig_ix >= n_script");
      return FS_E_INVALID;
    }
    const dim3 blk(kSeqBlock);
    FS_TRY(status.reserve(kStWords));
    FS_HIP(hipMemsetAsync(status.p, 0, kStWords * sizeof(uint32_t), s));
    a.status = status.p;
    hipLaunchKernelGGL(k_tr_check, dim3(blocks_of(a.n, kSeqBlock)), blk, 0, s, src, a);
    hipLaunchKernelGGL(k_tr_units_ok, dim3(blocks_of(a.n_script, kSeqBlock)), blk, 0, s, a);
    FS_HIP(hipGetLastError());
    FS_TRY(fs_runs_find(d_rows, a.n, a.min_words, max_gap, s, &runs, &a.heads, &a.n_runs));
    uint32_t st[kStWords];
    FS_HIP(hipMemcpyAsync(st, status.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    if (st[kStBadRecord]) {
      fs_set_error("a work >= n_works (%u) or an orig_ix >= n_script (%u)", a.n_works,
                   a.n_script);
      return FS_E_INVALID;
    }
    if (st[kStBadUnit]) {
      fs_set_error("a unit_of entry that is neither below n_units (%u) nor 0xFFFFFFFF",
                   a.n_units);
      return FS_E_INVALID;
    }

    // the sequence elements, in record order
    const uint32_t run_blocks = blocks_of(a.n_runs, kSeqBlock);
    FS_TRY(cnt.reserve(run_blocks));
    a.cnt = cnt.p;
    if (run_blocks) hipLaunchKernelGGL((k_tr_seq<false>), dim3(run_blocks), blk, 0, s, src, a);
    hipLaunchKernelGGL(k_tr_scan, dim3(1), dim3(kScanBlock), 0, s, a.cnt, a.cnt, run_blocks,
                       (unsigned long long*)nullptr, a.status + kStSeq);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(st, status.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    a.n_seq = st[kStSeq];
    if (!a.n_seq) return FS_OK;
    const size_t m = a.n_seq;
    FS_TRY(seq.reserve(6 * m));
    a.work = seq.p;
    a.ff = seq.p + m;
    a.fl = seq.p + 2 * m;
    a.of = seq.p + 3 * m;
    a.ol = seq.p + 4 * m;
    a.unit = seq.p + 5 * m;
    hipLaunchKernelGGL((k_tr_seq<true>), dim3(run_blocks), blk, 0, s, src, a);
    FS_HIP(hipGetLastError());
    return FS_OK;
  }
};

}  // namespace
