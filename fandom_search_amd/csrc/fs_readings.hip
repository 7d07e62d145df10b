// fs_readings.hip -- `ao3.py readings`: the wordings fans give each quoted stretch (fs_readings
// in include/fandom_search.h).  The passages of fs_passages, each taken as the sequence of
// (script offset, spelling) of its records, grouped into readings (equal sequences from the
// same script word on) and spans (equal first and last script word), the readings ranked
// inside their span.
//
// Nothing is sorted globally.  Readings are found with an open-addressing table keyed by a
// 64-bit hash of the sequence; equal hashes are settled by comparing the two sequences record
// by record, so the result does not depend on the hash (FS_READINGS_HASH_BITS cuts it down to
// prove that).  A reading's first passage is the atomicMin of its passages' numbers, which no
// schedule changes.  Distinct works are counted with the set primitive of fs_variants
// (fs_probe.h) over (reading, work) and (span, work).  Separate launches; no workgroup waits
// on another:
//   k_rd_check        one lane per record: work, orig_ix and spell in range
//   (fs_runs_find)    the run heads, as fs_passages joins them
//   k_rd_kept         one lane per run: kept runs counted per workgroup, then (after k_rd_scan)
//                     placed in record order as {first, length, orig_first, orig_last}
//   k_rd_insert       one wave per passage: lanes stride its records for the hash and for the
//                     comparisons; lane 0 claims slots and counts
//   k_rd_span_count / k_rd_scan / k_rd_span_scatter / k_rd_span_rank
//                     spans bucketed by orig_first, ordered by orig_last inside a bucket
//   k_rd_scan / k_rd_span_write   a span's first reading; the span records
//   k_rd_scatter / k_rd_rank      readings to their span, ranked there (a span of more than
//                     kLong readings, or a bucket of more than kLong spans, by the whole wave)
#include "fs_internal.h"
#include "fs_probe.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kLong = 64;

static_assert(sizeof(fs_reading) == 40 && sizeof(fs_reading_span) == 24, "fs_readings");

struct RdArgs {
  const uint32_t* work;
  const uint32_t* orig;
  const uint32_t* spell;
  const uint32_t* heads;         // [n_runs + 1]
  uint32_t n, n_runs, n_works, n_script, n_spell, min_words;
  uint32_t n_pass, n_spans, n_readings;
  uint64_t mask;                 // slots - 1 of each of the four tables
  uint64_t hash_mask;            // FS_READINGS_HASH_BITS: the bits of the sequence hash kept
  uint32_t* cnt;                 // [workgroups of runs] kept runs, then their exclusive scan
  uint4* pinfo;                  // [n_pass] {first record, records, orig_first, orig_last}
  uint32_t* pwork;               // [n_pass]
  unsigned long long* rd_tab;    // tag << 32 | passage that claimed the slot
  unsigned long long* sp_tab;    // orig_first << 32 | orig_last
  unsigned long long* rw_tab;    // reading slot << 32 | work
  unsigned long long* sw_tab;    // span slot << 32 | work
  uint32_t* rd_first;            // [slots] smallest passage of the reading
  uint32_t* rd_np;               //         its passages
  uint32_t* rd_nw;               //         its works
  uint32_t* rd_span;             //         its span's slot
  uint32_t* sp_np;               // [slots] passages of the span
  uint32_t* sp_nw;               //         its works
  uint32_t* sp_nr;               //         its readings
  uint32_t* sp_id;               //         its place in the output
  uint32_t* of_cnt;              // [n_script] spans that start at the word
  uint32_t* of_first;            //            the spans in front of them
  uint32_t* of_cur;              //            placed so far
  uint2* sp_tmp;                 // [n_spans] {slot, orig_last}, bucket by bucket, unordered
  uint32_t* sp_slot;             // [n_spans] slot of the span at that place
  uint32_t* sp_nrs;              //           its readings
  uint32_t* sp_firstr;           //           the readings in front of them
  uint32_t* sp_cur;              //           placed so far
  uint4* rd_tmp;                 // [n_readings] {first passage, passages, works, span}, unranked
  uint32_t* status;              // [0] invalid input, [1] total of the last scan
  fs_reading* readings;
  fs_reading_span* spans;
};

__global__ __launch_bounds__(kBlock) void k_rd_check(RdArgs a) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool bad = i < a.n && (a.work[i] >= a.n_works || a.orig[i] >= a.n_script ||
                               a.spell[i] >= a.n_spell);
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[0], 1u);
}

// exclusive scan of in[0..nb) into out (which may be in), *total = sum (one workgroup, chunks
// of 1024 in turn)
__global__ __launch_bounds__(kScanBlock) void k_rd_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t nb, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, nb, out, total);
}

// kPlace false: kept runs of this workgroup's 256 runs into cnt; true: the kept runs to their
// places, cnt holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_rd_kept(RdArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  uint32_t b = 0, e = 0;
  if (r < a.n_runs) {
    b = a.heads[r];
    e = a.heads[r + 1];
  }
  const bool keep = r < a.n_runs && e - b >= a.min_words;
  uint32_t rank, total;
  block_rank<kBlock>(keep, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = total;
  } else if (keep) {
    const uint32_t p = a.cnt[blockIdx.x] + rank;
    a.pinfo[p] = make_uint4(b, e - b, a.orig[b], a.orig[e - 1]);
    a.pwork[p] = a.work[b];
  }
}

// the slot of `key` in `tab`; true when this call put it there
__device__ inline bool set_insert(unsigned long long* tab, uint64_t mask, unsigned long long key,
                                  uint32_t* slot) {
  bool inserted;
  *slot = (uint32_t)fs_probe_insert(tab, mask, fs_mix64(key), key,
                                    [key](unsigned long long cur) { return cur == key; },
                                    &inserted);
  return inserted;
}

// the readings of passages x and y (wave-uniform) are equal; the whole wave compares
__device__ inline bool same_reading(const RdArgs& a, uint4 x, uint4 y, uint32_t lane) {
  if (x.y != y.y || x.z != y.z || x.w != y.w) return false;
  for (uint32_t c = 0; c < x.y; c += 64) {       // (equal orig_first: the offsets are equal
    const uint32_t i = c + lane;                 //  when the script indices are)
    const bool differ = i < x.y && (a.orig[x.x + i] != a.orig[y.x + i] ||
                                    a.spell[x.x + i] != a.spell[y.x + i]);
    if (__ballot(differ)) return false;
  }
  return true;
}

__global__ __launch_bounds__(kBlock) void k_rd_insert(RdArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (p >= a.n_pass) return;
  const uint4 me = a.pinfo[p];
  const uint32_t w = a.pwork[p];
  // a sum over the records of a mix of (position, offset, spelling): the order in which the
  // lanes' parts are added does not matter
  uint64_t acc = 0;
  for (uint32_t i = lane; i < me.y; i += 64) {
    const uint64_t rec = (uint64_t)(a.orig[me.x + i] - me.z) << 32 | a.spell[me.x + i];
    acc += fs_mix64(rec + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull);
  }
  acc = wave_sum(acc);
  uint64_t h = acc ^ fs_mix64((uint64_t)me.z << 32 | me.y);
  h = fs_mix64(fs_mix64(h) & a.hash_mask);       // the kept bits decide slot and tag
  const uint32_t tag = (uint32_t)(h >> 32);
  const unsigned long long mine = (unsigned long long)tag << 32 | p;

  uint32_t sslot = 0;
  if (lane == 0) {
    uint32_t other;
    set_insert(a.sp_tab, a.mask, (unsigned long long)me.z << 32 | me.w, &sslot);
    atomicAdd(&a.sp_np[sslot], 1u);
    if (set_insert(a.sw_tab, a.mask, (unsigned long long)sslot << 32 | w, &other))
      atomicAdd(&a.sp_nw[sslot], 1u);
  }
  sslot = (uint32_t)__builtin_amdgcn_readfirstlane((int)sslot);

  // the slot of this reading: lane 0 reads or claims, the wave compares (fs_probe.h's loop)
  uint64_t pos = h & a.mask;
  bool inserted = false;
  for (;; pos = (pos + 1) & a.mask) {
    unsigned long long cur = 0;
    if (lane == 0) {
      cur = __hip_atomic_load(&a.rd_tab[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kProbeEmpty) {
        cur = atomicCAS(&a.rd_tab[pos], kProbeEmpty, mine);
        if (cur == kProbeEmpty) cur = mine;
      }
    }
    cur = wave_first(cur);
    if (cur == mine) {
      inserted = true;
      break;
    }
    if ((uint32_t)(cur >> 32) == tag && same_reading(a, me, a.pinfo[(uint32_t)cur], lane)) break;
  }
  if (lane == 0) {
    const uint32_t rslot = (uint32_t)pos;
    uint32_t other;
    // a value read here is never below the slot's final one: a passage at or above it need not try
    if (p < __hip_atomic_load(&a.rd_first[rslot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMin(&a.rd_first[rslot], p);
    atomicAdd(&a.rd_np[rslot], 1u);
    if (set_insert(a.rw_tab, a.mask, (unsigned long long)rslot << 32 | w, &other))
      atomicAdd(&a.rd_nw[rslot], 1u);
    if (inserted) {
      a.rd_span[rslot] = sslot;
      atomicAdd(&a.sp_nr[sslot], 1u);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_rd_span_count(RdArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const unsigned long long key = a.sp_tab[slot];
  if (key != kProbeEmpty) atomicAdd(&a.of_cnt[(uint32_t)(key >> 32)], 1u);
}

__global__ __launch_bounds__(kBlock) void k_rd_span_scatter(RdArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  const unsigned long long key = a.sp_tab[slot];
  if (key == kProbeEmpty) return;
  const uint32_t o = (uint32_t)(key >> 32);
  a.sp_tmp[a.of_first[o] + atomicAdd(&a.of_cur[o], 1u)] = make_uint2((uint32_t)slot, (uint32_t)key);
}

// one lane per span: the spans of its bucket that end earlier are its place there
__global__ __launch_bounds__(kBlock) void k_rd_span_rank(RdArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool live = p < a.n_spans;
  uint2 c = make_uint2(0, 0);
  uint32_t first = 0, len = 0, rank = 0;
  if (live) {
    c = a.sp_tmp[p];
    const uint32_t o = (uint32_t)(a.sp_tab[c.x] >> 32);
    first = a.of_first[o];
    len = a.of_cnt[o];
  }
  const bool is_long = live && len > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)first, j);
    const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)len, j);
    const uint32_t yj = (uint32_t)__builtin_amdgcn_readlane((int)c.y, j);
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) before += a.sp_tmp[fj + k].y < yj ? 1u : 0u;
    before = wave_sum(before);
    if ((int)lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k) rank += a.sp_tmp[first + k].y < c.y ? 1u : 0u;
  if (live) {
    const uint32_t s = first + rank;
    a.sp_id[c.x] = s;
    a.sp_slot[s] = c.x;
    a.sp_nrs[s] = a.sp_nr[c.x];
  }
}

__global__ __launch_bounds__(kBlock) void k_rd_span_write(RdArgs a) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= a.n_spans) return;
  const uint32_t slot = a.sp_slot[s];
  const unsigned long long key = a.sp_tab[slot];
  a.spans[s] = fs_reading_span{(uint32_t)(key >> 32), (uint32_t)key, a.sp_np[slot], a.sp_nw[slot],
                               a.sp_nrs[s], a.sp_firstr[s]};
}

__global__ __launch_bounds__(kBlock) void k_rd_scatter(RdArgs a) {
  const uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot > a.mask) return;
  if (a.rd_tab[slot] == kProbeEmpty) return;
  const uint32_t s = a.sp_id[a.rd_span[slot]];
  a.rd_tmp[a.sp_firstr[s] + atomicAdd(&a.sp_cur[s], 1u)] =
      make_uint4(a.rd_first[slot], a.rd_np[slot], a.rd_nw[slot], s);
}

// x stands in front of y inside their span: {first passage, passages, works, span}
__device__ inline bool precedes(uint4 x, uint4 y) {
  if (x.z != y.z) return x.z > y.z;
  if (x.y != y.y) return x.y > y.y;
  return x.x < y.x;
}

__global__ __launch_bounds__(kBlock) void k_rd_rank(RdArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const bool live = p < a.n_readings;
  uint4 c = make_uint4(0, 0, 0, 0);
  uint32_t first = 0, len = 0, rank = 0;
  if (live) {
    c = a.rd_tmp[p];
    first = a.sp_firstr[c.w];
    len = a.sp_nrs[c.w];
  }
  const bool is_long = live && len > kLong;
  for (uint64_t lm = __ballot(is_long); lm; lm &= lm - 1) {
    const int j = __builtin_amdgcn_readfirstlane(__builtin_ctzll(lm));
    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)first, j);
    const uint32_t lj = (uint32_t)__builtin_amdgcn_readlane((int)len, j);
    uint4 cj;
    cj.x = (uint32_t)__builtin_amdgcn_readlane((int)c.x, j);
    cj.y = (uint32_t)__builtin_amdgcn_readlane((int)c.y, j);
    cj.z = (uint32_t)__builtin_amdgcn_readlane((int)c.z, j);
    cj.w = 0;                                                    // (not compared)
    uint32_t before = 0;
    for (uint32_t k = lane; k < lj; k += 64) before += precedes(a.rd_tmp[fj + k], cj) ? 1u : 0u;
    before = wave_sum(before);
    if ((int)lane == j) rank = before;
  }
  if (live && !is_long)
    for (uint32_t k = 0; k < len; ++k) rank += precedes(a.rd_tmp[first + k], c) ? 1u : 0u;
  if (live) {
    const uint4 info = a.pinfo[c.x];
    fs_reading r;
    r.first = info.x;
    r.orig_first = info.z;
    r.orig_last = info.w;
    r.n_words = info.y;
    r.n_passages = c.y;
    r.n_works = c.z;
    r.span = c.w;
    r.rank = rank + 1;
    r.reserved = 0;
    a.readings[first + rank] = r;
  }
}

uint64_t readings_hash_mask() {
  const char* e = getenv("FS_READINGS_HASH_BITS");   // diagnostic: k bits of the hash, 0: all collide
  if (!e || !*e) return ~0ull;
  const long k = strtol(e, nullptr, 10);
  return k <= 0 ? 0ull : k >= 64 ? ~0ull : (1ull << k) - 1;
}

struct RunsGuard {
  fs_runs* r = nullptr;
  ~RunsGuard() { if (r) fs_runs_free(r); }
};

// passages, tables, spans, readings, copy out, total of the last call
thread_local double t_ms[6];

}  // namespace

extern "C" int fs_readings(int device, const uint32_t* work, const uint32_t* fan_ix,
                           const uint32_t* orig_ix, const uint32_t* spell, uint64_t n_rows,
                           uint32_t n_works, uint32_t n_script, uint32_t n_spell,
                           uint32_t min_words, uint32_t max_gap, fs_reading* readings,
                           uint64_t cap_readings, fs_reading_span* spans, uint64_t cap_spans,
                           uint64_t* n_readings, uint64_t* n_spans, uint64_t* n_passages) {
  for (double& t : t_ms) t = 0.0;
  if (!n_readings || !n_spans || !n_passages || (cap_readings && !readings) ||
      (cap_spans && !spans)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0) {
    fs_set_error("min_words must be at least 1");
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("readings", n_rows, n_script));
  *n_readings = *n_spans = *n_passages = 0;
  if (n_rows == 0) return FS_OK;
  if (!work || !fan_ix || !orig_ix || !spell) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  const auto invalid = [] {
    fs_set_error("a work >= n_works, an orig_ix >= n_script or a spell >= n_spell");
    return FS_E_INVALID;
  };
  if (!n_works || !n_script || !n_spell) return invalid();
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  // raw columns, not fs_row records: the passes below read one column each
  DBuf<uint32_t> d_work, d_fan, d_orig, d_spell, d_status;
  FS_TRY(d_work.upload(work, n, nullptr));
  FS_TRY(d_fan.upload(fan_ix, n, nullptr));
  FS_TRY(d_orig.upload(orig_ix, n, nullptr));
  FS_TRY(d_spell.upload(spell, n, nullptr));
  FS_TRY(d_status.reserve(4));
  FS_HIP(hipMemsetAsync(d_status.p, 0, 4 * sizeof(uint32_t), nullptr));
  RdArgs a{};
  a.work = d_work.p;
  a.orig = d_orig.p;
  a.spell = d_spell.p;
  a.n = n;
  a.n_works = n_works;
  a.n_script = n_script;
  a.n_spell = n_spell;
  a.min_words = min_words;
  a.hash_mask = readings_hash_mask();
  a.status = d_status.p;
  Clock<6> clk;
  FS_TRY(clk.mark(0, nullptr));
  hipLaunchKernelGGL(k_rd_check, dim3(blocks_of(n, kBlock)), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  RunsGuard runs;
  FS_TRY(fs_runs_find_cols(d_work.p, d_fan.p, d_orig.p, n, min_words, max_gap, nullptr, &runs.r,
                           &a.heads, &a.n_runs));
  uint32_t st[2];
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  if (st[0]) return invalid();

  // the kept runs, in record order
  const uint32_t run_blocks = blocks_of(a.n_runs, kBlock);
  DBuf<uint32_t> d_cnt, d_pwork;
  DBuf<uint4> d_pinfo;
  FS_TRY(d_cnt.reserve(run_blocks));
  a.cnt = d_cnt.p;
  hipLaunchKernelGGL(k_rd_kept<false>, dim3(run_blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.cnt, a.cnt, run_blocks,
                     a.status + 1);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  a.n_pass = st[1];
  *n_passages = a.n_pass;
  if (!a.n_pass) return FS_OK;
  const uint64_t slots = fs_probe_slots(a.n_pass);
  if (slots * FS_READINGS_SLOT_BYTES > FS_READINGS_MAX_BYTES) {
    fs_set_error("%u passages: tables of more than %u bytes", a.n_pass, FS_READINGS_MAX_BYTES);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(d_pinfo.reserve(a.n_pass));
  FS_TRY(d_pwork.reserve(a.n_pass));
  a.pinfo = d_pinfo.p;
  a.pwork = d_pwork.p;
  hipLaunchKernelGGL(k_rd_kept<true>, dim3(run_blocks), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(1, nullptr));

  // readings and spans: tables and counts
  DBuf<unsigned long long> d_keys;               // the four key tables
  DBuf<uint32_t> d_first, d_zero;                // rd_first; the seven counters and ids per slot
  DBuf<uint32_t> d_of;                           // of_cnt, of_first, of_cur
  FS_TRY(d_keys.reserve(4 * slots));
  FS_TRY(d_first.reserve(slots));
  FS_TRY(d_zero.reserve(7 * slots));
  FS_TRY(d_of.reserve(3 * (size_t)n_script));
  FS_HIP(hipMemsetAsync(d_keys.p, 0xFF, 4 * slots * sizeof(unsigned long long), nullptr));
  FS_HIP(hipMemsetAsync(d_first.p, 0xFF, slots * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_zero.p, 0, 7 * slots * sizeof(uint32_t), nullptr));
  FS_HIP(hipMemsetAsync(d_of.p, 0, 3 * (size_t)n_script * sizeof(uint32_t), nullptr));
  a.mask = slots - 1;
  a.rd_tab = d_keys.p;
  a.sp_tab = d_keys.p + slots;
  a.rw_tab = d_keys.p + 2 * slots;
  a.sw_tab = d_keys.p + 3 * slots;
  a.rd_first = d_first.p;
  a.rd_np = d_zero.p;
  a.rd_nw = d_zero.p + slots;
  a.rd_span = d_zero.p + 2 * slots;
  a.sp_np = d_zero.p + 3 * slots;
  a.sp_nw = d_zero.p + 4 * slots;
  a.sp_nr = d_zero.p + 5 * slots;
  a.sp_id = d_zero.p + 6 * slots;
  a.of_cnt = d_of.p;
  a.of_first = d_of.p + n_script;
  a.of_cur = d_of.p + 2 * (size_t)n_script;
  const uint32_t slot_blocks = blocks_of(slots, kBlock);
  hipLaunchKernelGGL(k_rd_insert, dim3((a.n_pass + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock),
                     0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(2, nullptr));

  // spans in (orig_first, orig_last) order
  hipLaunchKernelGGL(k_rd_span_count, dim3(slot_blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.of_cnt, a.of_first,
                     n_script, a.status + 1);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  a.n_spans = st[1];
  *n_spans = a.n_spans;
  DBuf<uint2> d_sp_tmp;
  DBuf<uint32_t> d_sp;                           // sp_slot, sp_nrs, sp_firstr, sp_cur
  DBuf<fs_reading_span> d_spans;
  FS_TRY(d_sp_tmp.reserve(a.n_spans));
  FS_TRY(d_sp.reserve(4 * (size_t)a.n_spans));
  FS_TRY(d_spans.reserve(a.n_spans));
  FS_HIP(hipMemsetAsync(d_sp.p + 3 * (size_t)a.n_spans, 0, (size_t)a.n_spans * sizeof(uint32_t),
                        nullptr));
  a.sp_tmp = d_sp_tmp.p;
  a.sp_slot = d_sp.p;
  a.sp_nrs = d_sp.p + a.n_spans;
  a.sp_firstr = d_sp.p + 2 * (size_t)a.n_spans;
  a.sp_cur = d_sp.p + 3 * (size_t)a.n_spans;
  a.spans = d_spans.p;
  const uint32_t span_blocks = blocks_of(a.n_spans, kBlock);
  hipLaunchKernelGGL(k_rd_span_scatter, dim3(slot_blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rd_span_rank, dim3(span_blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rd_scan, dim3(1), dim3(kScanBlock), 0, nullptr, a.sp_nrs, a.sp_firstr,
                     a.n_spans, a.status + 1);
  hipLaunchKernelGGL(k_rd_span_write, dim3(span_blocks), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpy(st, d_status.p, sizeof st, hipMemcpyDeviceToHost));
  a.n_readings = st[1];
  *n_readings = a.n_readings;
  FS_TRY(clk.mark(3, nullptr));
  if (a.n_readings > cap_readings || a.n_spans > cap_spans) {
    fs_set_error("%u readings and %u spans need room", a.n_readings, a.n_spans);
    return FS_E_CAPACITY;
  }

  // readings to their span, ranked there
  DBuf<uint4> d_rd_tmp;
  DBuf<fs_reading> d_readings;
  FS_TRY(d_rd_tmp.reserve(a.n_readings));
  FS_TRY(d_readings.reserve(a.n_readings));
  a.rd_tmp = d_rd_tmp.p;
  a.readings = d_readings.p;
  hipLaunchKernelGGL(k_rd_scatter, dim3(slot_blocks), dim3(kBlock), 0, nullptr, a);
  hipLaunchKernelGGL(k_rd_rank, dim3(blocks_of(a.n_readings, kBlock)), dim3(kBlock), 0, nullptr, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, nullptr));
  FS_HIP(hipMemcpyAsync(readings, d_readings.p, (size_t)a.n_readings * sizeof(fs_reading),
                        hipMemcpyDeviceToHost, nullptr));
  FS_HIP(hipMemcpyAsync(spans, d_spans.p, (size_t)a.n_spans * sizeof(fs_reading_span),
                        hipMemcpyDeviceToHost, nullptr));
  FS_TRY(clk.mark(5, nullptr));
  FS_HIP(hipDeviceSynchronize());
  for (int k = 0; k < 5; ++k) t_ms[k] = clk.elapsed(k, k + 1);
  t_ms[5] = clk.elapsed(0, 5);
  return FS_OK;
}

extern "C" int fs_readings_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
