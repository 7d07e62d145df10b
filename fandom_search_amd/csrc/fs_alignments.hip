// fs_alignments.hip -- `ao3.py alignments`: quotes with inserted or dropped words, a gapped
// local alignment of every fan work against the script (fs_alignments, fs_alignments_rows in
// include/fandom_search.h).  Records sorted by (work, fan_ix); record j < i of the same work may
// precede i when the fan and the script index each step 1 .. R + 1 ahead, at the cost
// P * ((df - 1) + (do - 1)):
//   best(i) = S + max(0, max over such j of best(j) - cost(j, i)), prev(i) the largest j at a
//   maximum above 0, root(i) = root(prev(i)); a tree's peak is its smallest record with the
//   largest best, its alignment the path from the root to the peak.
// Candidates are compared as one 64-bit key, the value in the high half and j in the low half,
// peaks as (best, ~i): a plain maximum gives both tie rules whatever the order the candidates
// are looked at in.  Every output is an integer and no schedule changes it.
//
// Separate launches; no workgroup waits on another:
//   k_al_heads       one lane per record: the order check; a record starts a segment when its
//                    work changes or its fan index is more than R + 1 past the record before it
//                    (no link crosses such a step); heads counted per workgroup, then (after
//                    k_al_scan) placed
//   k_al_bin         one lane per segment: the segments of more than FS_ALIGNMENTS_SMALL records,
//                    counted per workgroup, then listed
//   k_al_chain_lane  a lane per segment of up to FS_ALIGNMENTS_SMALL records: the recurrence as
//                    it stands, over the records in reach
//   k_al_chain_wave  a wave per listed segment.  The last 64 records stay in registers, record i
//                    in lane (i - segment head) % 64 with its best, fan and script index and the
//                    path figures standing at it.  A step: every lane forms the value of its
//                    record, a DPP maximum and a ballot pick prev (the nearest lane at the
//                    maximum), the winner's figures come by readlane, and the lane of record i
//                    takes the new record over.  Candidates behind the ring (more than 64
//                    records in reach: records sharing a fan index) are read back from global
//                    memory, 64 per load, and that step takes one 64-bit wave maximum over the
//                    keys (value, j); FS_ALIGNMENTS_RING=0 takes every candidate that way.
//                    Both chain kernels carry n_words, n_exact, the skipped words and the pieces
//                    along prev, so the figures of an alignment stand at its peak; and a tree
//                    lies inside one segment, so the segment's own lane or wave keeps the peak
//                    and the size of its trees (the wave: once per 64 records and distinct root).
//   k_al_keep        one lane per record: a root whose peak has n_words >= M is kept; kept
//                    roots and their n_words counted per workgroup, then (after two scans) the
//                    alignments written in root order
//   k_al_trace       one lane per kept alignment: prev walked back from the peak,
//                    path[path_at + n_words(i) - 1] = i
#include "fs_internal.h"
#include "fs_prims.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kSmallDefault = 8;
constexpr uint32_t kRing = 64;                 // records a wave keeps in registers

static_assert(sizeof(fs_alignment) == 56, "fs_alignment");

// status words
enum { kStBad = 0, kStSegs = 1, kStWave = 2, kStKept = 3, kStPath = 4, kStWords = 8 };

typedef unsigned long long u64;

struct AlArgs {
  uint32_t n, n_seg, min_words, reach, match, gap;
  uint32_t small;                // the most records of a segment a single lane takes
  uint32_t ring;                 // kRing, or 0: every candidate through global memory
  uint32_t* cnt;                 // [workgroups of records] segment heads, then their scan
  uint32_t* heads;               // [n_seg + 1]
  uint32_t* bcnt;                // [workgroups of segments] wave-class segments, then their scan
  uint32_t* list;                // [n_seg] the wave-class segments
  uint32_t* best;                // [n] each: the recurrence ...
  uint32_t* prev;
  uint32_t* root;                //          ... and the figures of the path that ends here
  uint32_t* nw;
  uint32_t* nex;
  uint32_t* fsk;
  uint32_t* osk;
  uint32_t* pcs;
  u64* peak;                     // [n] at a root: (best, ~i) of its tree's peak
  uint32_t* size;                // [n] at a root: the records of its tree
  uint32_t* kcnt;                // [workgroups of records] kept roots, then their scan
  uint32_t* wcnt;                // [workgroups of records] their path records, then their scan
  uint32_t* status;
  fs_alignment* out;
  uint32_t* path;
};

// the figures of the path root .. i, carried along prev
struct Fig {
  uint32_t root, nw, nex, fsk, osk, pcs;
};

__device__ inline Fig fig_root(uint32_t i, bool exact) {
  return Fig{i, 1u, exact ? 1u : 0u, 0u, 0u, 1u};
}

// the path of p one link on, the fan index df and the script index dor ahead
__device__ inline Fig fig_next(Fig p, uint32_t df, uint32_t dor, bool exact) {
  return Fig{p.root, p.nw + 1, p.nex + (exact ? 1u : 0u), p.fsk + (df - 1), p.osk + (dor - 1),
             p.pcs + (df != 1 || dor != 1 ? 1u : 0u)};
}

// what a record at (fi, oi) gets from candidate j (best bj, fan fj, script oj); 0: not one
__device__ inline uint32_t cand_value(uint32_t fi, uint32_t oi, uint32_t fj, uint32_t oj,
                                      uint32_t bj, int64_t r1, int64_t gap) {
  const int64_t df = (int64_t)fi - (int64_t)fj, dor = (int64_t)oi - (int64_t)oj;
  if (df < 1 || df > r1 || dor < 1 || dor > r1) return 0;
  const int64_t v = (int64_t)bj - gap * (df + dor - 2);
  return v > 0 ? (uint32_t)v : 0u;
}

// the candidate's key: the value above j; 0 stays 0
__device__ inline u64 key_of(uint32_t value, uint32_t j) {
  return value ? (u64)value << 32 | j : 0;
}

__device__ inline u64 cand_key(uint32_t fi, uint32_t oi, uint32_t fj, uint32_t oj, uint32_t bj,
                               uint32_t j, int64_t r1, int64_t gap) {
  return key_of(cand_value(fi, oi, fj, oj, bj, r1, gap), j);
}

// one DPP step of a maximum: lanes the step does not write keep their own value (they read 0)
template <int kCtrl, int kRows>
__device__ inline uint32_t dpp_max(uint32_t x) {
  const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, kCtrl, kRows, 0xF, false);
  return y > x ? y : x;
}

// the largest value of the wave's 64 lanes, wave-uniform: six DPP steps leave it in lane 63
// (the steps of wave_sum_lane63 in fs_device.h), one readlane hands it round
__device__ inline uint32_t wave_max_u32(uint32_t x) {
  x = dpp_max<0xB1, 0xF>(x);                   // quad_perm [1,0,3,2]
  x = dpp_max<0x4E, 0xF>(x);                   // quad_perm [2,3,0,1]
  x = dpp_max<0x141, 0xF>(x);                  // row_half_mirror
  x = dpp_max<0x140, 0xF>(x);                  // row_mirror
  x = dpp_max<0x142, 0xA>(x);                  // row_bcast:15 into rows 1, 3
  x = dpp_max<0x143, 0xC>(x);                  // row_bcast:31 into rows 2, 3
  return lane_u32(x, 63);
}

__device__ inline u64 peak_key(uint32_t best, uint32_t i) {
  return (u64)best << 32 | (uint32_t)~i;
}

// kPlace false: the order check, and the segment heads of this workgroup's 256 records into
// cnt; true: the heads to their places, cnt holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_al_heads(RowsSrc src, AlArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  bool head = false, bad = false;
  if (i < a.n) {
    head = true;
    if (i) {
      const uint4 s = src.key(i), r = src.key(i - 1);
      bad = s.x < r.x || (s.x == r.x && s.y < r.y);
      head = s.x != r.x || (uint64_t)s.y - (uint64_t)r.y > (uint64_t)a.reach + 1;
    }
  }
  uint32_t rank, total;
  block_rank<kBlock>(head, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = total;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&a.status[kStBad], 1u);
  } else {
    if (head) a.heads[a.cnt[blockIdx.x] + rank] = (uint32_t)i;
    if (i == 0) a.heads[a.n_seg] = a.n;
  }
}

// exclusive scan of in[0..nb) into out (which may be in), *total = sum (one workgroup, chunks
// of 1024 in turn)
__global__ __launch_bounds__(kScanBlock) void k_al_scan(const uint32_t* in, uint32_t* out,
                                                        uint32_t nb, uint32_t* total) {
  scan_array<uint32_t, uint32_t>(in, nb, out, total);
}

// kPlace false: the wave-class segments of this workgroup's 256 segments into bcnt; true: the
// segments to the list, bcnt holding the scan
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_al_bin(AlArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  const bool wave = k < a.n_seg && a.heads[k + 1] - a.heads[k] > a.small;
  uint32_t rank, total;
  block_rank<kBlock>(wave, s_w, &rank, &total);
  if (!kPlace) {
    if (threadIdx.x == 0) a.bcnt[blockIdx.x] = total;
  } else if (wave) {
    a.list[a.bcnt[blockIdx.x] + rank] = k;
  }
}

// a lane per segment of 1 .. small records: the recurrence as it stands.  The lane reads back
// only what it wrote itself.
__global__ __launch_bounds__(kBlock) void k_al_chain_lane(RowsSrc src, AlArgs a) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= a.n_seg) return;
  const uint32_t b = a.heads[k], e = a.heads[k + 1];
  if (e - b > a.small) return;
  const int64_t r1 = (int64_t)a.reach + 1, gap = a.gap;
  for (uint32_t i = b; i < e; ++i) {
    const uint4 s = src.key(i);
    const bool exact = src.comb(i) <= 0.0;
    u64 key = 0;
    uint32_t pf = 0, po = 0;                            // the candidate held in key
    for (uint32_t j = i; j-- > b;) {
      const uint4 q = src.key(j);
      if ((int64_t)s.y - (int64_t)q.y > r1) break;      // (the fan index only falls from here)
      const u64 cand = cand_key(s.y, s.z, q.y, q.z, a.best[j], j, r1, gap);
      if (cand > key) {
        key = cand;
        pf = q.y;
        po = q.z;
      }
    }
    const uint32_t j = (uint32_t)key, bi = a.match + (uint32_t)(key >> 32);
    const Fig f = key ? fig_next(Fig{a.root[j], a.nw[j], a.nex[j], a.fsk[j], a.osk[j], a.pcs[j]},
                                 s.y - pf, s.z - po, exact)
                      : fig_root(i, exact);
    a.best[i] = bi;
    a.prev[i] = key ? j : FS_NONE;
    a.root[i] = f.root;
    a.nw[i] = f.nw;
    a.nex[i] = f.nex;
    a.fsk[i] = f.fsk;
    a.osk[i] = f.osk;
    a.pcs[i] = f.pcs;
    const u64 pk = peak_key(bi, i);
    if (!key) {
      a.size[i] = 1;
      a.peak[i] = pk;
    } else {
      a.size[f.root] += 1;
      if (pk > a.peak[f.root]) a.peak[f.root] = pk;
    }
  }
}

__device__ inline u64 lane_u64(u64 v, uint32_t s) {                 // s wave-uniform
  return (u64)lane_u32((uint32_t)(v >> 32), s) << 32 | lane_u32((uint32_t)v, s);
}

// a wave (= a workgroup) per listed segment
__global__ __launch_bounds__(64) void k_al_chain_wave(RowsSrc src, AlArgs a) {
  const uint32_t lane = threadIdx.x;
  const uint32_t k = a.list[blockIdx.x];
  const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.heads[k]);
  const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.heads[k + 1]);
  const int64_t r1 = (int64_t)a.reach + 1, gap = a.gap;
  // the ring: this lane's record, the latest i with (i - b) % 64 == lane
  bool r_has = false;
  uint32_t r_ix = 0, r_fan = 0, r_orig = 0, r_best = 0;
  Fig r_fig{0u, 0u, 0u, 0u, 0u, 0u};
  for (uint32_t t0 = b; t0 < e; t0 += 64) {
    const uint32_t m = e - t0 < 64 ? e - t0 : 64u;
    const bool live = lane < m;
    const uint32_t mine = t0 + lane;
    const uint4 tk = live ? src.key(mine) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t tex = live && src.comb(mine) <= 0.0 ? 1u : 0u;
    // is the nearest record behind the ring in reach of `mine`?  (the fan index only falls
    // from there, so if it is not, none behind it is)
    const int64_t far = (int64_t)mine - 1 - (int64_t)a.ring;
    const bool tfar = live && far >= (int64_t)b &&
                      (int64_t)tk.y - (int64_t)src.key((uint64_t)far).y <= r1;
    const u64 far_mask = __ballot(tfar);
    for (uint32_t s = 0; s < m; ++s) {
      const uint32_t i = t0 + s;
      const uint32_t fi = lane_u32(tk.y, s), oi = lane_u32(tk.z, s);
      const bool exact = lane_u32(tex, s) != 0;
      const uint32_t value =
          a.ring && r_has ? cand_value(fi, oi, r_fan, r_orig, r_best, r1, gap) : 0u;
      u64 key = 0;
      if (!((far_mask >> s) & 1)) {
        // every candidate is in the ring: the largest value by DPP, and among the lanes that
        // hold it the nearest record -- lane s - 1 holds record i - 1, lane s - 2 record i - 2
        // and so on round the ring, so with lane l moved to bit (l - s) % 64 it is the top bit
        const uint32_t top = wave_max_u32(value);
        if (top) {
          const u64 at = __ballot(value == top);
          const u64 turned = s ? at >> s | at << (64 - s) : at;
          key = key_of(top, i - 1 - (uint32_t)__builtin_clzll(turned));
        }
      } else {
        key = key_of(value, r_ix);
        __threadfence();                                // this wave's stores, before it reads them back
        for (int64_t near = (int64_t)i - 1 - (int64_t)a.ring;; near -= 64) {
          const int64_t j = near - (int64_t)lane;
          bool in = false;
          if (j >= (int64_t)b) {
            const uint4 q = src.key((uint64_t)j);
            in = (int64_t)fi - (int64_t)q.y <= r1;
            if (in) {
              const u64 cand = cand_key(fi, oi, q.y, q.z, ld_agent(a.best + j), (uint32_t)j, r1,
                                        gap);
              if (cand > key) key = cand;
            }
          }
          if (!((__ballot(in) >> 63) & 1)) break;       // the farthest of the 64 out of reach
        }
        key = wave_first(wave_max(key));
      }
      const uint32_t j = (uint32_t)key, bi = a.match + (uint32_t)(key >> 32);
      Fig f = fig_root(i, exact);
      if (key) {
        Fig p;
        uint32_t pf, po;
        if (a.ring && i - j <= kRing) {                 // the winner is in the ring
          const uint32_t wl = (j - b) & 63;
          pf = lane_u32(r_fan, wl);
          po = lane_u32(r_orig, wl);
          p = Fig{lane_u32(r_fig.root, wl), lane_u32(r_fig.nw, wl), lane_u32(r_fig.nex, wl),
                  lane_u32(r_fig.fsk, wl), lane_u32(r_fig.osk, wl), lane_u32(r_fig.pcs, wl)};
        } else {
          // behind the fence above.  Every lane loads the same words; taking them as scalars
          // ends the loads here, so the steps that stay in the ring never wait on memory
          const uint4 q = src.key(j);
          pf = wave_first(q.y);
          po = wave_first(q.z);
          p = Fig{wave_first(ld_agent(a.root + j)), wave_first(ld_agent(a.nw + j)),
                  wave_first(ld_agent(a.nex + j)), wave_first(ld_agent(a.fsk + j)),
                  wave_first(ld_agent(a.osk + j)), wave_first(ld_agent(a.pcs + j))};
        }
        f = fig_next(p, fi - pf, oi - po, exact);
      }
      if (lane == s) {
        r_has = true;
        r_ix = i;
        r_fan = fi;
        r_orig = oi;
        r_best = bi;
        r_fig = f;
        st_agent(a.best + i, bi);
        st_agent(a.prev + i, key ? j : FS_NONE);
        st_agent(a.root + i, f.root);
        st_agent(a.nw + i, f.nw);
        st_agent(a.nex + i, f.nex);
        st_agent(a.fsk + i, f.fsk);
        st_agent(a.osk + i, f.osk);
        st_agent(a.pcs + i, f.pcs);
      }
    }
    // the tile's records stand in lanes 0 .. m - 1: per distinct root, its first lane adds
    // their number and their peak to the tree's (size and peak start at 0)
    const u64 pk = peak_key(r_best, r_ix);
    uint32_t same = 0;
    u64 top = 0;
    bool leader = live;
    for (uint32_t t = 0; t < m; ++t) {
      const uint32_t rt = lane_u32(r_fig.root, t);
      const u64 kt = lane_u64(pk, t);
      if (live && rt == r_fig.root) {
        same += 1;
        if (kt > top) top = kt;
        if (t < lane) leader = false;
      }
    }
    if (leader) {
      atomicAdd(a.size + r_fig.root, same);
      atomicMax(a.peak + r_fig.root, top);
    }
  }
}

// kPlace false: the kept roots of this workgroup's 256 records and their path records into
// kcnt and wcnt; true: the alignments to their places, kcnt and wcnt holding the scans
template <bool kPlace>
__global__ __launch_bounds__(kBlock) void k_al_keep(AlArgs a) {
  __shared__ uint32_t s_w[kBlock / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  uint32_t p = 0, words = 0;
  if (i < a.n && a.prev[i] == FS_NONE) {
    p = ~(uint32_t)a.peak[i];
    words = a.nw[p];
  }
  const bool keep = words && words >= a.min_words;
  if (!keep) words = 0;
  uint32_t rank, total, wtotal;
  block_rank<kBlock>(keep, s_w, &rank, &total);
  const uint32_t wpre = block_scan<kBlock>(words, s_w, &wtotal);
  if (!kPlace) {
    if (threadIdx.x == 0) {
      a.kcnt[blockIdx.x] = total;
      a.wcnt[blockIdx.x] = wtotal;
    }
  } else if (keep) {
    fs_alignment x;
    x.first = i;
    x.last = p;
    x.n_words = words;
    x.n_exact = a.nex[p];
    x.score = a.best[p];
    x.fan_skipped = a.fsk[p];
    x.orig_skipped = a.osk[p];
    x.pieces = a.pcs[p];
    x.tree_records = a.size[i];
    x.reserved = 0;
    x.path_at = (uint64_t)a.wcnt[blockIdx.x] + wpre;
    a.out[a.kcnt[blockIdx.x] + rank] = x;
  }
}

__global__ __launch_bounds__(kBlock) void k_al_trace(AlArgs a, uint32_t n_kept) {
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= n_kept) return;
  const uint64_t at = a.out[x].path_at;
  for (uint32_t i = (uint32_t)a.out[x].last; i != FS_NONE; i = a.prev[i])
    a.path[at + a.nw[i] - 1] = i;
}

// segments, bins, chain, keep, trace, total of the last call
thread_local double t_ms[6];

struct AlScratch {
  DBuf<uint32_t> status, cnt, heads, bcnt, list, rec, size, kw;
  DBuf<u64> peak;
};

// the rules both entry points share; *done when nothing is left to do
int al_check(uint64_t n_rows, uint32_t min_words, uint32_t reach, uint32_t match, uint32_t gap,
             const void* out, uint64_t cap, uint64_t* n_out, const void* path, uint64_t path_cap,
             uint64_t* n_path, bool* done) {
  *done = false;
  if (!n_out || !n_path || (cap && !out) || (path_cap && !path)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || match == 0 || reach > 63 || match > 16 || gap > 16) {
    fs_set_error("min_words and match must be at least 1, reach at most 63, match and gap at "
                 "most 16");
    return FS_E_INVALID;
  }
  if (n_rows >= (1ull << 32) || n_rows * match >= (1ull << 32)) {
    fs_set_error("%llu records at match %u: alignments take scores below 2^32",
                 (unsigned long long)n_rows, match);
    return FS_E_UNSUPPORTED;
  }
  *n_out = 0;
  *n_path = 0;
  for (double& t : t_ms) t = 0.0;
  *done = n_rows == 0;
  return FS_OK;
}

// *n_out and *n_path set; d_out and d_path written unless FS_E_CAPACITY (all on `s`, finished
// on return)
int al_run(const fs_row* d_rows, uint32_t n, uint32_t min_words, uint32_t reach, uint32_t match,
           uint32_t gap, fs_alignment* d_out, uint64_t cap, uint64_t* n_out, uint32_t* d_path,
           uint64_t path_cap, uint64_t* n_path, hipStream_t s) {
  const RowsSrc src{d_rows};
  AlScratch k;
  AlArgs a{};
  Clock<6> clk;
  a.n = n;
  a.min_words = min_words;
  a.reach = reach;
  a.match = match;
  a.gap = gap;
  // FS_ALIGNMENTS_SMALL, FS_ALIGNMENTS_RING: diagnostics, read on each call
  a.small = env_u32("FS_ALIGNMENTS_SMALL", kSmallDefault, 0xFFFFFFFFu);
  a.ring = env_u32("FS_ALIGNMENTS_RING", 1, 1) ? kRing : 0u;
  a.out = d_out;
  a.path = d_path;
  const dim3 blk(kBlock);
  const uint32_t rec_blocks = blocks_of(n, kBlock);
  FS_TRY(k.status.reserve(kStWords));
  FS_TRY(k.cnt.reserve(rec_blocks));
  FS_HIP(hipMemsetAsync(k.status.p, 0, kStWords * sizeof(uint32_t), s));
  a.status = k.status.p;
  a.cnt = k.cnt.p;
  FS_TRY(clk.mark(0, s));

  // the segments
  hipLaunchKernelGGL((k_al_heads<false>), dim3(rec_blocks), blk, 0, s, src, a);
  hipLaunchKernelGGL(k_al_scan, dim3(1), dim3(kScanBlock), 0, s, a.cnt, a.cnt, rec_blocks,
                     a.status + kStSegs);
  FS_HIP(hipGetLastError());
  uint32_t st[kStWords];
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  if (st[kStBad]) {
    fs_set_error("records are not sorted by (work, fan_ix)");
    return FS_E_INVALID;
  }
  a.n_seg = st[kStSegs];
  const uint32_t seg_blocks = blocks_of(a.n_seg, kBlock);
  FS_TRY(k.heads.reserve((size_t)a.n_seg + 1));
  FS_TRY(k.bcnt.reserve(seg_blocks));
  FS_TRY(k.list.reserve(a.n_seg));
  a.heads = k.heads.p;
  a.bcnt = k.bcnt.p;
  a.list = k.list.p;
  hipLaunchKernelGGL((k_al_heads<true>), dim3(rec_blocks), blk, 0, s, src, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(1, s));

  // the segments by class
  hipLaunchKernelGGL(k_al_bin<false>, dim3(seg_blocks), blk, 0, s, a);
  hipLaunchKernelGGL(k_al_scan, dim3(1), dim3(kScanBlock), 0, s, a.bcnt, a.bcnt, seg_blocks,
                     a.status + kStWave);
  hipLaunchKernelGGL(k_al_bin<true>, dim3(seg_blocks), blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  const uint32_t n_wave = st[kStWave];
  FS_TRY(clk.mark(2, s));

  // the chains
  const size_t nn = n;
  FS_TRY(k.rec.reserve(8 * nn));
  FS_TRY(k.size.reserve(nn));
  FS_TRY(k.peak.reserve(nn));
  FS_TRY(k.kw.reserve(2 * (size_t)rec_blocks));
  a.best = k.rec.p;
  a.prev = k.rec.p + nn;
  a.root = k.rec.p + 2 * nn;
  a.nw = k.rec.p + 3 * nn;
  a.nex = k.rec.p + 4 * nn;
  a.fsk = k.rec.p + 5 * nn;
  a.osk = k.rec.p + 6 * nn;
  a.pcs = k.rec.p + 7 * nn;
  a.size = k.size.p;
  a.peak = k.peak.p;
  a.kcnt = k.kw.p;
  a.wcnt = k.kw.p + rec_blocks;
  FS_HIP(hipMemsetAsync(a.size, 0, nn * sizeof(uint32_t), s));
  FS_HIP(hipMemsetAsync(a.peak, 0, nn * sizeof(u64), s));
  if (a.small)
    hipLaunchKernelGGL(k_al_chain_lane, dim3(seg_blocks), blk, 0, s, src, a);
  if (n_wave) hipLaunchKernelGGL(k_al_chain_wave, dim3(n_wave), dim3(64), 0, s, src, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(3, s));

  // the kept alignments, in root order
  hipLaunchKernelGGL(k_al_keep<false>, dim3(rec_blocks), blk, 0, s, a);
  hipLaunchKernelGGL(k_al_scan, dim3(1), dim3(kScanBlock), 0, s, a.kcnt, a.kcnt, rec_blocks,
                     a.status + kStKept);
  hipLaunchKernelGGL(k_al_scan, dim3(1), dim3(kScanBlock), 0, s, a.wcnt, a.wcnt, rec_blocks,
                     a.status + kStPath);
  FS_HIP(hipGetLastError());
  FS_HIP(hipMemcpyAsync(st, k.status.p, sizeof st, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  const uint32_t n_kept = st[kStKept], n_words = st[kStPath];
  *n_out = n_kept;
  *n_path = n_words;
  const bool fits = n_kept <= cap && n_words <= path_cap;
  if (fits && n_kept) hipLaunchKernelGGL(k_al_keep<true>, dim3(rec_blocks), blk, 0, s, a);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(4, s));
  if (fits && n_kept)
    hipLaunchKernelGGL(k_al_trace, dim3(blocks_of(n_kept, kBlock)), blk, 0, s, a, n_kept);
  FS_HIP(hipGetLastError());
  FS_TRY(clk.mark(5, s));
  FS_HIP(hipStreamSynchronize(s));
  for (int j = 0; j < 5; ++j) t_ms[j] = clk.elapsed(j, j + 1);
  t_ms[5] = clk.elapsed(0, 5);
  if (!fits) {
    fs_set_error("%u alignments and %u path records need room", n_kept, n_words);
    return FS_E_CAPACITY;
  }
  return FS_OK;
}

}  // namespace

extern "C" int fs_alignments(int device, const uint32_t* work, const uint32_t* fan_ix,
                             const uint32_t* orig_ix, const double* comb, uint64_t n_rows,
                             uint32_t min_words, uint32_t reach, uint32_t match, uint32_t gap,
                             fs_alignment* out, uint64_t cap, uint64_t* n_out, uint32_t* path,
                             uint64_t path_cap, uint64_t* n_path) {
  bool done = false;
  FS_TRY(al_check(n_rows, min_words, reach, match, gap, out, cap, n_out, path, path_cap, n_path,
                  &done));
  if (done) return FS_OK;
  if (!work || !fan_ix || !orig_ix || !comb) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_alignment> d_out;
  DBuf<uint32_t> d_path;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n, nullptr, comb));
  const uint64_t most = n_rows / min_words;                  // alignments never outnumber this
  FS_TRY(d_out.reserve(cap < most ? cap : most));
  FS_TRY(d_path.reserve(path_cap < n_rows ? path_cap : n_rows));   // nor path records the records
  const int rc = al_run(rows.p, n, min_words, reach, match, gap, d_out.p, cap, n_out, d_path.p,
                        path_cap, n_path, nullptr);
  if (rc != FS_OK) return rc;
  if (*n_out) FS_TRY(copy_out(out, d_out, *n_out));
  if (*n_path) FS_TRY(copy_out(path, d_path, *n_path));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_alignments_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                  uint32_t min_words, uint32_t reach, uint32_t match,
                                  uint32_t gap, fs_alignment* d_out, uint64_t cap,
                                  uint64_t* n_out, uint32_t* d_path, uint64_t path_cap,
                                  uint64_t* n_path) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  bool done = false;
  FS_TRY(al_check(n_rows, min_words, reach, match, gap, d_out, cap, n_out, d_path, path_cap,
                  n_path, &done));
  if (done) return FS_OK;
  if (!d_rows || ((uintptr_t)d_rows & 15) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_path & 3)) {
    fs_set_error("d_rows must be a 16-byte aligned device pointer, d_out 8-byte, d_path 4-byte");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  return al_run(d_rows, (uint32_t)n_rows, min_words, reach, match, gap, d_out, cap, n_out, d_path,
                path_cap, n_path, ix->stream);
}

extern "C" int fs_alignments_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
