// fs_clusters.hip -- `ao3.py clusters`: families of fan works quoting the same lines
// (fs_clusters, fs_clusters_rows in include/fandom_search.h).  Two active works are linked when
// their coverages share enough words (min_shared, min_jaccard); a family is a connected
// component of the links.  The links come from the tile product of fs_pairs.hip and are united
// where they are found: no pair is ever written to memory.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   CoverJob (fs_tiles.h)  run heads, check, active numbering, coverage matrix, row popcounts
//   k_clusters_init     one lane per row of the matrix: every work its own parent
//   k_clusters_links    the link pass.  The workgroups and the staged product of
//                       k_pairs_tiles<0>; a link adds to `links` of both works, offers itself
//                       as their `best` and unites them in the parent array (uf_unite)
//   k_clusters_flatten  one lane per active work: its root into `root`, an array of its own;
//                       the size, the links and the hub of the family gathered at the root
//   k_clusters_flag     one lane per active work: a root of >= min_size works is listed
//   k_pairs_scan        the listed families numbered in root order; later their offsets
//   k_clusters_heads    one lane per listed root: root and size of its number
//   k_clusters_members  one lane per active work: placed behind its family's cursor, a copy
//                       of the offsets (the offsets themselves stay as scanned)
//   k_clusters_works    one lane per work: its fs_cluster_work
//   k_clusters_depth    a wave per (listed family, 64 script words): lane j counts the members
//                       that cover word 64 k + j; covered, common and peak to the family by
//                       atomics, the 64-bit mask of words at depth >= t kept
//   k_clusters_merge    a wave per listed family: the longest run of its masks (a lane a
//                       stretch of them, the stretches merged: prefix, suffix, best run), its
//                       fs_cluster
//
// The parent array is over active numbers, which ascend with the work numbers.  uf_unite hooks
// the larger root under the smaller one with a compare-and-swap on the larger root's own entry,
// so parent[x] <= x always, an entry that has left itself never returns, and the last root of a
// component is its smallest work in whatever order the links are met.  A lost CAS means that
// another lane hooked that root first: both finds are taken again, which is progress of the
// whole, not a wait for anyone.  Path halving stores an ancestor over an ancestor: a stale
// store lengthens a path, it never leaves the component.  That is all the link pass needs, but
// it does not make `parent[i]` a root at any given time: a halving store of another wave may
// land on an entry after its owner has looked its root up.  So k_clusters_flatten writes what it
// finds into `root`, which no find ever stores to, and every later kernel reads `root` alone.
#include "fs_tiles.h"
#include "fs_unionfind.h"

namespace {

struct ClusterArgs : CoverArgs {
  uint32_t min_jaccard, min_size, common_pct, n_listed;
  uint32_t* links;              // [rows] links of an active work
  unsigned long long* best;     // [rows] shared << 32 | (0xFFFFFFFF - partner)
  uint32_t* parent;             // [rows] union-find: an ancestor, not always the root
  uint32_t* root;               // [rows] k_clusters_flatten: the root (written once each)
  uint32_t* size;               // [rows] at a root: works of the family
  unsigned long long* linksum;  // [rows] at a root: the members' links, summed
  unsigned long long* hub;      // [rows] at a root: links << 32 | (0xFFFFFFFF - active number)
  uint32_t* listed;             // [rows] 1 at a listed root
  uint32_t* num;                // [rows] the scan of `listed`: the number of a listed root
  uint32_t* members;            // [n_active] active numbers by listed family
  uint32_t* fam_root;           // [n_listed] active number of the root
  uint32_t* fam_size;           // [n_listed]
  uint32_t* fam_off;            // [n_listed] first member
  uint32_t* fam_cur;            // [n_listed] k_clusters_members: the cursor, from fam_off
  uint32_t* fam_cnt;            // [n_listed][2] covered, common
  unsigned long long* fam_peak; // [n_listed] depth << 32 | (0xFFFFFFFF - word)
  unsigned long long* mask;     // [n_listed][nk] words at depth >= t
  fs_cluster_work* works;
  fs_cluster* clusters;
};

__global__ __launch_bounds__(kRunBlock) void k_clusters_init(ClusterArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < a.n_tiles * kTile) a.parent[i] = i;
}

// shared words `sh` of works covering ca and cb words: a link?
__device__ inline bool is_link(const ClusterArgs& a, uint32_t sh, uint32_t ca, uint32_t cb) {
  return sh >= a.min_shared && 100u * sh >= a.min_jaccard * (ca + cb - sh);
}

// blockIdx.x = row tile * n_chunks + chunk, as k_pairs_tiles
__global__ __launch_bounds__(kBlock) void k_clusters_links(ClusterArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ uint32_t s_wa[kTile], s_wb[kTile], s_ca[kTile], s_cb[kTile];
  const uint32_t ti = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const uint32_t tj0 = ti > c * kChunk ? ti : c * kChunk;
  const uint32_t tj1 = (c + 1) * kChunk < a.n_tiles ? (c + 1) * kChunk : a.n_tiles;
  if (tj0 >= tj1) return;                                // below the diagonal
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kTile) {
    s_wa[threadIdx.x] = a.work_of[(size_t)ti * kTile + threadIdx.x];
    s_ca[threadIdx.x] = a.covered[(size_t)ti * kTile + threadIdx.x];
  }
  for (uint32_t tj = tj0; tj < tj1; ++tj) {
    __syncthreads();                                     // s_wb, s_cb and s_sh of the tile before
    if (threadIdx.x < kTile) {
      s_wb[threadIdx.x] = a.work_of[(size_t)tj * kTile + threadIdx.x];
      s_cb[threadIdx.x] = a.covered[(size_t)tj * kTile + threadIdx.x];
    }
    tile_counts(a, ti, tj, s_a, s_b, s_sh);
    const bool diag = tj == ti;
    // rows: wave w takes rows 16 w .. 16 w + 15, a lane per column
    bool any = false;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const bool keep = is_link(a, sh, s_ca[r], s_cb[lane]) && (!diag || r < lane);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      any = true;
      const unsigned long long key =
          wave_max(keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - s_wb[lane]) : 0ull);
      if (lane == 0) {
        atomicAdd(&a.links[(size_t)ti * kTile + r], (uint32_t)__popcll(m));
        atomicMax(&a.best[(size_t)ti * kTile + r], key);
      }
      if (keep) uf_unite(a.parent, ti * kTile + r, tj * kTile + lane);
    }
    // columns: wave w takes columns 16 w .. 16 w + 15, a lane per row
    if (!__syncthreads_or(any)) continue;
    for (uint32_t cc = 0; cc < kTile / 4; ++cc) {
      const uint32_t col = wave * (kTile / 4) + cc;
      const uint32_t sh = s_sh[lane * kShStride + col];
      const bool keep = is_link(a, sh, s_ca[lane], s_cb[col]) && (!diag || lane < col);
      const uint64_t m = __ballot(keep);
      if (!m) continue;
      const unsigned long long key =
          wave_max(keep ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - s_wa[lane]) : 0ull);
      if (lane == 0) {
        atomicAdd(&a.links[(size_t)tj * kTile + col], (uint32_t)__popcll(m));
        atomicMax(&a.best[(size_t)tj * kTile + col], key);
      }
    }
  }
}

// One lane per active work.  No link is made any more, so the roots stand and every walk ends
// at the root of its component whatever the halving stores of other lanes do to the paths
// meanwhile; the result goes to root[i], which only this lane writes.
__global__ __launch_bounds__(kRunBlock) void k_clusters_flatten(ClusterArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active) return;
  const uint32_t r = uf_find(a.parent, i);
  a.root[i] = r;
  const uint32_t l = a.links[i];
  atomicAdd(&a.size[r], 1u);
  if (l) {
    atomicAdd(&a.linksum[r], (unsigned long long)l);
    atomicMax(&a.hub[r], ((unsigned long long)l << 32) | (0xFFFFFFFFu - i));
  }
}

__global__ __launch_bounds__(kRunBlock) void k_clusters_flag(ClusterArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active) return;
  a.listed[i] = a.root[i] == i && a.size[i] >= a.min_size;
}

__global__ __launch_bounds__(kRunBlock) void k_clusters_heads(ClusterArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active || !a.listed[i]) return;
  a.fam_root[a.num[i]] = i;
  a.fam_size[a.num[i]] = a.size[i];
}

// The order of a family's members plays no part: what is taken over them is sums and maxima
// of integers.
__global__ __launch_bounds__(kRunBlock) void k_clusters_members(ClusterArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active) return;
  const uint32_t r = a.root[i];
  if (a.listed[r]) a.members[atomicAdd(&a.fam_cur[a.num[r]], 1u)] = i;
}

// one lane per work; flag: nullptr when no work is active
__global__ __launch_bounds__(kRunBlock) void k_clusters_works(ClusterArgs a, const uint32_t* flag) {
  const uint64_t w = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (w >= a.n_works) return;
  uint4 lo = make_uint4(0u, FS_NONE, 0u, FS_NONE), hi = make_uint4(0u, FS_NONE, 0u, 0u);
  if (flag && flag[w]) {
    const uint32_t i = a.act[w], r = a.root[i];
    lo = make_uint4(a.covered[i], a.work_of[r], a.size[r], a.listed[r] ? a.num[r] : FS_NONE);
    hi.x = a.links[i];
    if (hi.x) {
      const unsigned long long b = a.best[i];
      hi.y = 0xFFFFFFFFu - (uint32_t)b;
      hi.z = (uint32_t)(b >> 32);
    }
  }
  uint4* o = reinterpret_cast<uint4*>(a.works + w);
  o[0] = lo;
  o[1] = hi;
}

// A wave per (listed family f, 64-bit word k of the rows).  The members are taken 64 at a
// time, a lane a member's word (one load each; neighbours in a family are mostly neighbours
// in a tile), and the words that hold anything handed round the wave.
__global__ __launch_bounds__(kBlock) void k_clusters_depth(ClusterArgs a) {
  const uint64_t id = (uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (id >= (uint64_t)a.n_listed * a.nk) return;         // (a whole wave leaves)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t f = (uint32_t)(id / a.nk), k = (uint32_t)(id % a.nk);
  const uint32_t n = a.fam_size[f];
  const uint32_t* mem = a.members + a.fam_off[f];
  uint32_t depth = 0;
  for (uint32_t m0 = 0; m0 < n; m0 += 64) {
    unsigned long long x = 0;
    if (m0 + lane < n) {
      const uint32_t i = mem[m0 + lane];
      x = a.cov[((size_t)(i / kTile) * a.nk + k) * kTile + i % kTile];
    }
    uint64_t any = __ballot(x != 0);
    while (any) {
      const int src = __builtin_ctzll(any);
      any &= any - 1;
      depth += (uint32_t)(__shfl(x, src) >> lane) & 1u;
    }
  }
  const unsigned long long t = ((unsigned long long)a.common_pct * n + 99) / 100;
  const uint64_t cov = __ballot(depth >= 1), com = __ballot(depth >= t);
  const unsigned long long peak =
      wave_max(((unsigned long long)depth << 32) | (0xFFFFFFFFu - (k * 64 + lane)));
  if (lane) return;
  a.mask[(size_t)f * a.nk + k] = com;
  if (!cov) return;
  atomicAdd(&a.fam_cnt[2 * f], (uint32_t)__popcll(cov));
  if (com) atomicAdd(&a.fam_cnt[2 * f + 1], (uint32_t)__popcll(com));
  atomicMax(&a.fam_peak[f], peak);
}

// A stretch of script words: its first word and length, the set words at its start and its
// end, and its longest run of set words (the first among equals).
struct Stretch {
  uint32_t start, len, pre, suf, best, best_at;
};

__device__ inline Stretch stretch_of(unsigned long long x, uint32_t base) {
  Stretch s{base, 64u, 0u, 0u, 0u, 0u};
  if (x == ~0ull) {
    s.pre = s.suf = s.best = 64u;
    s.best_at = base;
    return s;
  }
  s.pre = (uint32_t)__builtin_ctzll(~x);
  s.suf = (uint32_t)__builtin_clzll(~x);
  while (x) {
    const uint32_t at = (uint32_t)__builtin_ctzll(x);
    const uint32_t l = (uint32_t)__builtin_ctzll(~(x >> at));    // (x >> at has a clear bit)
    if (l > s.best) {
      s.best = l;
      s.best_at = base + at;
    }
    x = at + l >= 64 ? 0ull : x & (~0ull << (at + l));
  }
  return s;
}

// p then q, adjacent; an empty stretch (len 0) is the identity
__device__ inline Stretch stretch_merge(const Stretch& p, const Stretch& q) {
  if (!q.len) return p;
  if (!p.len) return q;
  Stretch s{p.start, p.len + q.len, p.pre == p.len ? p.len + q.pre : p.pre,
            q.suf == q.len ? q.len + p.suf : q.suf, p.best, p.best_at};
  if (p.suf + q.pre > s.best) {                          // in order of their first words:
    s.best = p.suf + q.pre;                              // a later run has to be longer
    s.best_at = q.start - p.suf;
  }
  if (q.best > s.best) {
    s.best = q.best;
    s.best_at = q.best_at;
  }
  return s;
}

__device__ inline Stretch stretch_shfl_down(const Stretch& s, uint32_t d) {
  return Stretch{__shfl_down(s.start, d), __shfl_down(s.len, d), __shfl_down(s.pre, d),
                 __shfl_down(s.suf, d), __shfl_down(s.best, d), __shfl_down(s.best_at, d)};
}

// a wave per listed family
__global__ __launch_bounds__(kBlock) void k_clusters_merge(ClusterArgs a) {
  const uint32_t f = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (f >= a.n_listed) return;                           // (a whole wave leaves)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t per = (a.nk + 63) / 64;
  const unsigned long long* mask = a.mask + (size_t)f * a.nk;
  Stretch s{0u, 0u, 0u, 0u, 0u, 0u};
  for (uint32_t k = lane * per; k < (lane + 1) * per && k < a.nk; ++k)
    s = stretch_merge(s, stretch_of(mask[k], k * 64));
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const Stretch o = stretch_shfl_down(s, d);
    if (lane % (2 * d) == 0) s = stretch_merge(s, o);
  }
  if (lane) return;
  const uint32_t r = a.fam_root[f];
  const unsigned long long hub = a.hub[r], peak = a.fam_peak[f], half = a.linksum[r] / 2;
  uint4* o = reinterpret_cast<uint4*>(a.clusters + f);
  o[0] = make_uint4(a.work_of[r], a.fam_size[f], half > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)half,
                    a.work_of[hub ? 0xFFFFFFFFu - (uint32_t)hub : r]);
  o[1] = make_uint4((uint32_t)(hub >> 32), a.fam_cnt[2 * f], a.fam_cnt[2 * f + 1],
                    (uint32_t)(peak >> 32));
  o[2] = make_uint4(0xFFFFFFFFu - (uint32_t)peak, s.best ? s.best_at : FS_NONE, s.best, 0u);
}

// coverage, links, families (flatten to the works), depth, merge of the last call
thread_local double t_ms[5];

// one call: families() through the per-work results and the number of listed families, then
// write()
struct ClustersJob {
  CoverJob cj;
  DBuf<uint32_t> links, parent, root, size, listed, num, members, fam_root, fam_size, fam_off,
      fam_cur, fam_cnt;
  DBuf<unsigned long long> best, linksum, hub, fam_peak, mask;
  Clock<8> clk;
  ClusterArgs a{};

  // d_works written, a.n_listed set (all on `s`, finished on return)
  int families(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
               uint32_t min_words, uint32_t max_gap, uint32_t min_shared, uint32_t min_jaccard,
               uint32_t min_size, uint32_t common_pct, fs_cluster_work* d_works, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.min_shared = min_shared;
    a.min_jaccard = min_jaccard;
    a.min_size = min_size;
    a.common_pct = common_pct;
    a.works = d_works;
    const dim3 work_grid((n_works + kRunBlock - 1) / kRunBlock), blk(kRunBlock);
    if (n) FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) {
      if (n_works) hipLaunchKernelGGL(k_clusters_works, work_grid, blk, 0, s, a, nullptr);
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));
      return FS_OK;
    }
    // the rows of the matrix and, at most, a row of masks per family of min_size works
    const uint64_t bytes = ((uint64_t)a.n_active + a.n_active / min_size) * a.nk * 8;
    if (bytes > FS_CLUSTERS_MAX_BYTES) {
      fs_set_error("%u works with a passage over %u script words in families of %u or more: "
                   "coverage and family rows of more than %u bytes", a.n_active, n_script,
                   min_size, FS_CLUSTERS_MAX_BYTES);
      return FS_E_UNSUPPORTED;
    }
    const size_t rows = (size_t)a.n_tiles * kTile;
    const uint64_t blocks = (uint64_t)a.n_tiles * a.n_chunks;
    if (blocks > 0x7FFFFFFFull) {
      fs_set_error("%u works with a passage: more tiles of pairs than a launch takes",
                   a.n_active);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(cj.reserve(a, s));
    FS_TRY(links.reserve(rows));
    FS_TRY(best.reserve(rows));
    FS_TRY(parent.reserve(rows));
    FS_TRY(root.reserve(rows));
    FS_TRY(size.reserve(rows));
    FS_TRY(linksum.reserve(rows));
    FS_TRY(hub.reserve(rows));
    FS_TRY(listed.reserve(rows));
    FS_TRY(num.reserve(rows));
    FS_TRY(members.reserve(rows));
    FS_HIP(hipMemsetAsync(links.p, 0, rows * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(best.p, 0, rows * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(size.p, 0, rows * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(linksum.p, 0, rows * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(hub.p, 0, rows * sizeof(unsigned long long), s));
    a.links = links.p;
    a.best = best.p;
    a.parent = parent.p;
    a.root = root.p;
    a.size = size.p;
    a.linksum = linksum.p;
    a.hub = hub.p;
    a.listed = listed.p;
    a.num = num.p;
    a.members = members.p;
    const dim3 row_grid((uint32_t)((rows + kRunBlock - 1) / kRunBlock));
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    hipLaunchKernelGGL(k_clusters_init, row_grid, blk, 0, s, a);
    FS_TRY(clk.mark(1, s));
    hipLaunchKernelGGL(k_clusters_links, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
    FS_TRY(clk.mark(2, s));
    hipLaunchKernelGGL(k_clusters_flatten, row_grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_clusters_flag, row_grid, blk, 0, s, a);
    hipLaunchKernelGGL(k_pairs_scan<uint32_t>, dim3(1), dim3(kScanBlock), 0, s, listed.p,
                       (uint64_t)a.n_active, num.p, cj.status.p + 2);
    hipLaunchKernelGGL(k_clusters_works, work_grid, blk, 0, s, a, cj.flag.p);
    FS_TRY(clk.mark(3, s));
    FS_HIP(hipGetLastError());
    uint32_t st[3];
    FS_HIP(hipMemcpyAsync(st, cj.status.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    a.n_listed = st[2];
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    t_ms[2] = clk.elapsed(2, 3);
    return FS_OK;
  }

  // the a.n_listed families into d_clusters (finished on return)
  int write(fs_cluster* d_clusters, hipStream_t s) {
    if (!a.n_listed) return FS_OK;
    {
      const size_t nf = a.n_listed;
      a.clusters = d_clusters;
      FS_TRY(fam_root.reserve(nf));
      FS_TRY(fam_size.reserve(nf));
      FS_TRY(fam_off.reserve(nf));
      FS_TRY(fam_cur.reserve(nf));
      FS_TRY(fam_cnt.reserve(2 * nf));
      FS_TRY(fam_peak.reserve(nf));
      FS_TRY(mask.reserve(nf * a.nk));
      FS_HIP(hipMemsetAsync(fam_cnt.p, 0, 2 * nf * sizeof(uint32_t), s));
      FS_HIP(hipMemsetAsync(fam_peak.p, 0, nf * sizeof(unsigned long long), s));
      a.fam_root = fam_root.p;
      a.fam_size = fam_size.p;
      a.fam_off = fam_off.p;
      a.fam_cur = fam_cur.p;
      a.fam_cnt = fam_cnt.p;
      a.fam_peak = fam_peak.p;
      a.mask = mask.p;
      const dim3 row_grid((a.n_active + kRunBlock - 1) / kRunBlock), blk(kRunBlock);
      const uint64_t waves = (uint64_t)nf * a.nk;       // <= FS_CLUSTERS_MAX_BYTES / 8
      FS_TRY(clk.mark(4, s));
      hipLaunchKernelGGL(k_clusters_heads, row_grid, blk, 0, s, a);
      hipLaunchKernelGGL(k_pairs_scan<uint32_t>, dim3(1), dim3(kScanBlock), 0, s, fam_size.p,
                         (uint64_t)nf, fam_off.p, cj.status.p + 3);
      FS_HIP(hipMemcpyAsync(fam_cur.p, fam_off.p, nf * sizeof(uint32_t),
                            hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(k_clusters_members, row_grid, blk, 0, s, a);
      FS_TRY(clk.mark(5, s));
      hipLaunchKernelGGL(k_clusters_depth, dim3((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64))),
                         dim3(kBlock), 0, s, a);
      FS_TRY(clk.mark(6, s));
      hipLaunchKernelGGL(k_clusters_merge, dim3((uint32_t)((nf + kBlock / 64 - 1) / (kBlock / 64))),
                         dim3(kBlock), 0, s, a);
      FS_TRY(clk.mark(7, s));
      FS_HIP(hipGetLastError());
    }
    FS_HIP(hipStreamSynchronize(s));
    t_ms[2] += clk.elapsed(4, 5);                        // (the member lists)
    t_ms[3] = clk.elapsed(5, 6);
    t_ms[4] = clk.elapsed(6, 7);
    return FS_OK;
  }
};

// the rules both entry points share
int clusters_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
                   uint32_t min_shared, uint32_t min_jaccard, uint32_t min_size,
                   uint32_t common_pct, const void* works, const void* clusters, uint64_t cap,
                   uint64_t* n_clusters) {
  if (!n_clusters || (n_works && !works) || (cap && !clusters)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_shared == 0 || min_size == 0 || common_pct == 0) {
    fs_set_error("min_words, min_shared, min_size and common_pct must be at least 1");
    return FS_E_INVALID;
  }
  if (min_jaccard > 100 || common_pct > 100) {
    fs_set_error("min_jaccard and common_pct are percentages: at most 100");
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("clusters", n_rows, n_script));
  *n_clusters = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_clusters(int device, const uint32_t* work, const uint32_t* fan_ix,
                           const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                           uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                           uint32_t min_shared, uint32_t min_jaccard, uint32_t min_size,
                           uint32_t common_pct, fs_cluster_work* works, fs_cluster* clusters,
                           uint64_t cap, uint64_t* n_clusters) {
  FS_TRY(clusters_check(n_rows, n_works, n_script, min_words, min_shared, min_jaccard, min_size,
                        common_pct, works, clusters, cap, n_clusters));
  if (!n_rows) {
    const fs_cluster_work none{0u, FS_NONE, 0u, FS_NONE, 0u, FS_NONE, 0u, 0u};
    for (uint32_t w = 0; w < n_works; ++w) works[w] = none;
    return FS_OK;
  }
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_cluster_work> d_works;
  DBuf<fs_cluster> d_clusters;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  FS_TRY(d_works.reserve(n_works));
  ClustersJob job;
  FS_TRY(job.families(rows.p, n, n_works, n_script, min_words, max_gap, min_shared, min_jaccard,
                      min_size, common_pct, d_works.p, nullptr));
  if (n_works) FS_TRY(copy_out(works, d_works, n_works));
  *n_clusters = job.a.n_listed;
  if (job.a.n_listed > cap) return FS_E_CAPACITY;
  FS_TRY(d_clusters.reserve(job.a.n_listed));
  FS_TRY(job.write(d_clusters.p, nullptr));
  if (job.a.n_listed) FS_TRY(copy_out(clusters, d_clusters, job.a.n_listed));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_clusters_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                                uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                                uint32_t min_shared, uint32_t min_jaccard, uint32_t min_size,
                                uint32_t common_pct, fs_cluster_work* d_works,
                                fs_cluster* d_clusters, uint64_t cap, uint64_t* n_clusters) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: clusters take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(clusters_check(n_rows, n_works, (uint32_t)ix->n_script, min_words, min_shared,
                        min_jaccard, min_size, common_pct, d_works, d_clusters, cap, n_clusters));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_works & 15) ||
      ((uintptr_t)d_clusters & 15)) {
    fs_set_error("d_rows, d_works and d_clusters must be 16-byte aligned device pointers");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  ClustersJob job;
  FS_TRY(job.families(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                      min_shared, min_jaccard, min_size, common_pct, d_works, ix->stream));
  *n_clusters = job.a.n_listed;
  if (job.a.n_listed > cap) return FS_E_CAPACITY;
  return job.write(d_clusters, ix->stream);
}

extern "C" int fs_clusters_times(double* ms) {
  return times_out(ms, t_ms, 5);
}
