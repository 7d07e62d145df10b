// fs_tree.hip -- `ao3.py tree`: how the families of works merge as the bar drops (fs_tree,
// fs_tree_rows in include/fandom_search.h).  The single-linkage dendrogram of the active works
// is the maximum spanning forest of the work x work similarity, replayed in the order of its
// edges.  The forest is built by Boruvka's rounds over the tile product of fs_pairs.hip: every
// family picks its first edge to another family, the picked edges are united, and a round costs
// one product.  No pair is ever written to memory; what is written is the forest, at most one
// edge per work.
//
// Every output is an integer, so partial results merge in any order.  Separate launches; no
// workgroup waits on another:
//   CoverJob (fs_tiles.h)  run heads, check, active numbering, coverage matrix, row popcounts
//   k_tree_init      one lane per row of the matrix: every work its own parent
//   per round
//   k_tree_flatten   one lane per row: its root into `root`, an array of its own, and the
//                    round's tables cleared
//   k_tree_best      the workgroups and the staged product of k_pairs_tiles<0>; a cell whose two
//                    works are in different families and that is an edge offers level << 32 |
//                    ~partner to both works, one 64-bit atomicMax per row per tile
//   k_tree_level     one lane per active work: its best level offered to its root
//   k_tree_choose    one lane per active work that holds its root's level: ~a << 32 | ~b of its
//                    edge offered to its root
//   k_tree_hook      one lane per root with a choice: uf_unite, and the lane whose
//                    compare-and-swap joins two families appends the edge
//   the host reads the number of edges; no new edge, or one fewer than works, ends the rounds
//   k_tree_detail    one lane per edge: the shared words and their longest run
//   the host sorts the edges and replays them (Replay): sides, sizes, levels, ranks, leaves
//
// The order of the edges -- level descending, then a, then b -- is strict, so the forest is the
// only one and the picked edges of a round hold no cycle: on a cycle of picks every family
// would prefer its pick to the pick that reaches it, all the way round.  Two families that pick
// the same edge are one edge met twice, and the second unite finds one root.  For one work,
// "highest level, then smallest partner" is its first edge: a smaller partner below the work
// is a smaller a, and any partner below it comes before every partner above it.  Over the works
// of a family the comparison has to be the whole (level, a, b), which k_tree_level and
// k_tree_choose make in two steps of one atomicMax each.
//
// The roots a round compares are those k_tree_flatten wrote: fs_unionfind.h on why `parent`
// itself is no root at a given time.  Between k_tree_hook and the next k_tree_flatten lies a
// kernel boundary, so every find of a flatten ends at a root that stands.
#include <algorithm>
#include <chrono>

#include "fs_tiles.h"
#include "fs_unionfind.h"

namespace {

struct TreeArgs : CoverArgs {
  uint32_t measure, min_level;
  uint32_t* parent;             // [rows] union-find: an ancestor, not always the root
  uint32_t* root;               // [rows] k_tree_flatten: the root at the start of the round
  unsigned long long* best;     // [rows] level << 32 | (0xFFFFFFFF - partner), 0: no edge
  uint32_t* cmax;               // [rows] at a root: the highest level a member holds
  unsigned long long* ckey;     // [rows] at a root: (0xFFFFFFFF - a) << 32 | (0xFFFFFFFF - b)
  uint4* edges;                 // [rows][2] a, b, level, 0; shared, run_first, run_words, 0
  uint32_t* n_edges;
};

__global__ __launch_bounds__(kRunBlock) void k_tree_init(TreeArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i < a.n_tiles * kTile) a.parent[i] = i;
}

// One lane per row of the matrix, the padding too (a root of its own: it shares nothing).
__global__ __launch_bounds__(kRunBlock) void k_tree_flatten(TreeArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_tiles * kTile) return;
  a.root[i] = uf_find(a.parent, i);
  a.best[i] = 0ull;
  a.cmax[i] = 0u;
  a.ckey[i] = 0ull;
}

// What a cell of `sh` shared words between works covering ca and cb offers to a work whose best
// level so far is `have`: level << 32 | ~partner, or 0 when it is no edge or lies below `have`.
// The Jaccard level is floor(sh * 10^6 / either); below max(have, min_level) it can be told
// without the division, so only a cell that could win or tie divides.  (sh >= 1: either >= 1.)
__device__ inline unsigned long long tree_offer(const TreeArgs& a, uint32_t sh, uint32_t ca,
                                               uint32_t cb, uint32_t have, uint32_t partner) {
  const uint32_t least = have > a.min_level ? have : a.min_level;
  uint32_t level = sh;
  if (a.measure == FS_TREE_JACCARD) {
    const unsigned long long num = (unsigned long long)sh * 1000000ull, either = ca + cb - sh;
    if (num < (unsigned long long)least * either) return 0ull;
    level = (uint32_t)(num / either);
  } else if (level < least) {
    return 0ull;
  }
  return ((unsigned long long)level << 32) | (0xFFFFFFFFu - partner);
}

__device__ inline uint32_t tree_level_now(const unsigned long long* best) {
  return (uint32_t)(__hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
}

// blockIdx.x = row tile * n_chunks + chunk, as k_pairs_tiles.  The level a work holds already
// is read once per tile: an older value rejects less, never more.
__global__ __launch_bounds__(kBlock) void k_tree_best(TreeArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ uint32_t s_ca[kTile], s_cb[kTile], s_ra[kTile], s_rb[kTile], s_ha[kTile], s_hb[kTile];
  const uint32_t ti = blockIdx.x / a.n_chunks, c = blockIdx.x % a.n_chunks;
  const uint32_t tj0 = ti > c * kChunk ? ti : c * kChunk;
  const uint32_t tj1 = (c + 1) * kChunk < a.n_tiles ? (c + 1) * kChunk : a.n_tiles;
  if (tj0 >= tj1) return;                                // below the diagonal
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kTile) {
    s_ca[threadIdx.x] = a.covered[(size_t)ti * kTile + threadIdx.x];
    s_ra[threadIdx.x] = a.root[(size_t)ti * kTile + threadIdx.x];
  }
  for (uint32_t tj = tj0; tj < tj1; ++tj) {
    __syncthreads();                                     // the tables and s_sh of the tile before
    if (threadIdx.x < kTile) {
      s_cb[threadIdx.x] = a.covered[(size_t)tj * kTile + threadIdx.x];
      s_rb[threadIdx.x] = a.root[(size_t)tj * kTile + threadIdx.x];
      s_ha[threadIdx.x] = tree_level_now(a.best + (size_t)ti * kTile + threadIdx.x);
      s_hb[threadIdx.x] = tree_level_now(a.best + (size_t)tj * kTile + threadIdx.x);
    }
    tile_counts(a, ti, tj, s_a, s_b, s_sh);
    const bool diag = tj == ti;
    // rows: wave w takes rows 16 w .. 16 w + 15, a lane per column
    bool any = false;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const bool cell = sh >= a.min_shared && s_ra[r] != s_rb[lane] && (!diag || r < lane);
      if (!__ballot(cell)) continue;
      any = true;
      const unsigned long long key = wave_max(
          cell ? tree_offer(a, sh, s_ca[r], s_cb[lane], s_ha[r], tj * kTile + lane) : 0ull);
      if (lane == 0 && key) atomicMax(&a.best[(size_t)ti * kTile + r], key);
    }
    // columns: wave w takes columns 16 w .. 16 w + 15, a lane per row
    if (!__syncthreads_or(any)) continue;
    for (uint32_t cc = 0; cc < kTile / 4; ++cc) {
      const uint32_t col = wave * (kTile / 4) + cc;
      const uint32_t sh = s_sh[lane * kShStride + col];
      const bool cell = sh >= a.min_shared && s_ra[lane] != s_rb[col] && (!diag || lane < col);
      if (!__ballot(cell)) continue;
      const unsigned long long key = wave_max(
          cell ? tree_offer(a, sh, s_ca[lane], s_cb[col], s_hb[col], ti * kTile + lane) : 0ull);
      if (lane == 0 && key) atomicMax(&a.best[(size_t)tj * kTile + col], key);
    }
  }
}

__global__ __launch_bounds__(kRunBlock) void k_tree_level(TreeArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active) return;
  const unsigned long long b = a.best[i];
  if (b) atomicMax(&a.cmax[a.root[i]], (uint32_t)(b >> 32));
}

__global__ __launch_bounds__(kRunBlock) void k_tree_choose(TreeArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active) return;
  const unsigned long long b = a.best[i];
  const uint32_t r = a.root[i];
  if (!b || (uint32_t)(b >> 32) != a.cmax[r]) return;
  const uint32_t p = 0xFFFFFFFFu - (uint32_t)b;
  const uint32_t lo = i < p ? i : p, hi = i < p ? p : i;
  atomicMax(&a.ckey[r], ((unsigned long long)(0xFFFFFFFFu - lo) << 32) | (0xFFFFFFFFu - hi));
}

// One lane per root with a choice.  The edges of a forest over n_active works are fewer than
// the rows of the matrix; the bound on `at` is there so that nothing else could be written to.
__global__ __launch_bounds__(kRunBlock) void k_tree_hook(TreeArgs a) {
  const uint32_t i = blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= a.n_active || a.root[i] != i) return;
  const unsigned long long k = a.ckey[i];
  if (!k) return;
  const uint32_t lo = 0xFFFFFFFFu - (uint32_t)(k >> 32), hi = 0xFFFFFFFFu - (uint32_t)k;
  if (lo >= a.n_active || hi >= a.n_active || !uf_unite(a.parent, lo, hi)) return;
  const uint32_t at = atomicAdd(a.n_edges, 1u);
  if (at < a.n_tiles * kTile) a.edges[2 * (size_t)at] = make_uint4(lo, hi, a.cmax[i], 0u);
}

// one lane per edge: what its two rows share (shared_run, fs_tiles.h)
__global__ __launch_bounds__(kRunBlock) void k_tree_detail(TreeArgs a, uint32_t n_edges) {
  const uint32_t e = blockIdx.x * kRunBlock + threadIdx.x;
  if (e >= n_edges) return;
  const uint4 head = a.edges[2 * (size_t)e];
  const SharedRun r =
      shared_run(a.cov + (size_t)(head.x / kTile) * a.nk * kTile + head.x % kTile,
                 a.cov + (size_t)(head.y / kTile) * a.nk * kTile + head.y % kTile, a.nk);
  a.edges[2 * (size_t)e + 1] = make_uint4(r.shared, r.run_first, r.run_words, 0u);
}

// cover, flatten, best, choose, hook, detail, replay, total of the last call; hooking rounds
thread_local double t_ms[9];

double host_ms(std::chrono::steady_clock::time_point from) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - from).count();
}

// The host's part: the edges of the forest, in active numbers, sorted and taken one by one
// (Kruskal over the forest alone keeps every edge, in the order Kruskal over all edges would).
// Sequential by nature and at most one step per work.
struct Replay {
  std::vector<fs_tree_work> works;
  std::vector<fs_tree_merge> merges;
  std::vector<fs_tree_level> levels;

  void none(uint32_t n_works) {
    const fs_tree_work w{0u, FS_NONE, 0u, 0u, FS_NONE, 0u, FS_NONE, FS_NONE};
    works.assign(n_works, w);
    merges.clear();
    levels.clear();
  }

  // edges[2 e], edges[2 e + 1] as k_tree_hook and k_tree_detail wrote them
  int run(uint32_t n_works, uint32_t n_active, const std::vector<uint32_t>& work_of,
          const std::vector<uint32_t>& covered, std::vector<uint4>& edges) {
    none(n_works);
    const uint32_t n_edges = (uint32_t)(edges.size() / 2);
    std::vector<uint32_t> order(n_edges);
    for (uint32_t e = 0; e < n_edges; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
      const uint4 &x = edges[2 * (size_t)p], &y = edges[2 * (size_t)q];
      if (x.z != y.z) return x.z > y.z;
      if (x.x != y.x) return x.x < y.x;
      return x.y < y.y;
    });
    std::vector<uint32_t> parent(n_active), size(n_active, 1u), first(n_active),
        last(n_active, FS_NONE);
    for (uint32_t i = 0; i < n_active; ++i) parent[i] = first[i] = i;
    auto find = [&](uint32_t x) {
      uint32_t r = x;
      while (parent[r] != r) r = parent[r];
      while (parent[x] != r) {
        const uint32_t up = parent[x];
        parent[x] = r;
        x = up;
      }
      return r;
    };
    for (uint32_t i = 0; i < n_active; ++i) works[work_of[i]].covered = covered[i];
    merges.resize(n_edges);
    uint32_t families = 0, largest = 0, singles = n_active;
    for (uint32_t k = 0; k < n_edges; ++k) {
      const uint4 head = edges[2 * (size_t)order[k]], tail = edges[2 * (size_t)order[k] + 1];
      const uint32_t fa = find(head.x), fb = find(head.y);
      if (fa == fb) {
        fs_set_error("tree: an edge inside one family in the replay");
        return FS_E_DEVICE;
      }
      const uint32_t sa = size[fa], sb = size[fb];
      const uint32_t lead = first[fa] < first[fb] ? first[fa] : first[fb];
      merges[k] = fs_tree_merge{work_of[head.x], work_of[head.y], head.z, tail.x, covered[head.x],
                                covered[head.y], last[fa], last[fb], sa, sb, sa + sb,
                                work_of[lead], 0u, tail.y, tail.z, 0u};
      parent[fb] = fa;
      size[fa] = sa + sb;
      first[fa] = lead;
      last[fa] = k;
      for (const uint32_t end : {head.x, head.y}) {
        fs_tree_work& w = works[work_of[end]];
        if (w.edges++ == 0) {
          w.joined_merge = k;
          w.joined_level = head.z;
          w.best = work_of[end == head.x ? head.y : head.x];
        }
      }
      families += 1u - (sa >= 2) - (sb >= 2);
      singles -= (sa == 1) + (sb == 1);
      if (sa + sb > largest) largest = sa + sb;
      if (levels.empty() || levels.back().level != head.z)
        levels.push_back(fs_tree_level{head.z, 0u, k, 0u, 0u, 0u, 0u, 0u});
      fs_tree_level& l = levels.back();
      l.merges += 1;
      l.families = families;
      l.largest = largest;
      l.joined = n_active - singles;
      l.singles = singles;
    }
    // the trees: most works first, then the earliest work
    std::vector<uint32_t> roots;
    for (uint32_t i = 0; i < n_active; ++i)
      if (find(i) == i) roots.push_back(i);
    std::sort(roots.begin(), roots.end(), [&](uint32_t p, uint32_t q) {
      return size[p] != size[q] ? size[p] > size[q] : first[p] < first[q];
    });
    std::vector<uint32_t> rank(n_active, 0u);
    for (uint32_t t = 0; t < roots.size(); ++t) rank[roots[t]] = t;
    for (uint32_t i = 0; i < n_active; ++i) {
      const uint32_t r = find(i);
      works[work_of[i]].tree = rank[r];
      works[work_of[i]].tree_works = size[r];
    }
    for (fs_tree_merge& m : merges) m.tree = works[m.a].tree;
    // the leaves, by a stack of its own (a path of works is as deep as it is long): a node is a
    // merge, or an active number with the top bit set (n_active < 2^25 under FS_TREE_MAX_BYTES)
    const uint32_t kWork = 0x80000000u;
    std::vector<uint32_t> stack;
    uint32_t leaf = 0;
    for (const uint32_t r : roots) {
      stack.push_back(last[r] == FS_NONE ? (kWork | r) : last[r]);
      while (!stack.empty()) {
        const uint32_t node = stack.back();
        stack.pop_back();
        if (node & kWork) {
          works[work_of[node & ~kWork]].leaf = leaf++;
          continue;
        }
        const fs_tree_merge& m = merges[node];
        const uint4 head = edges[2 * (size_t)order[node]];
        stack.push_back(m.right == FS_NONE ? (kWork | head.y) : m.right);
        stack.push_back(m.left == FS_NONE ? (kWork | head.x) : m.left);
      }
    }
    return FS_OK;
  }
};

// one call: everything up to the three record kinds on the host (finished on return)
struct TreeJob {
  CoverJob cj;
  DBuf<uint32_t> parent, root, cmax, n_edges;
  DBuf<unsigned long long> best, ckey;
  DBuf<uint4> edges;
  Clock<8> clk;
  TreeArgs a{};
  Replay out;

  int run(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
          uint32_t min_words, uint32_t max_gap, uint32_t measure, uint32_t min_shared,
          uint32_t min_level, hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.min_shared = min_shared;
    a.measure = measure;
    a.min_level = min_level;
    out.none(n_works);
    if (n) FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) return FS_OK;
    if ((uint64_t)a.n_active * ((uint64_t)a.nk * 8 + FS_TREE_ROW_BYTES) > FS_TREE_MAX_BYTES) {
      fs_set_error("%u works with a passage over %u script words: coverage rows and per-work "
                   "tables of more than %u bytes", a.n_active, n_script, FS_TREE_MAX_BYTES);
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
    FS_TRY(parent.reserve(rows));
    FS_TRY(root.reserve(rows));
    FS_TRY(best.reserve(rows));
    FS_TRY(cmax.reserve(rows));
    FS_TRY(ckey.reserve(rows));
    FS_TRY(edges.reserve(2 * rows));
    FS_TRY(n_edges.reserve(1));
    FS_HIP(hipMemsetAsync(n_edges.p, 0, sizeof(uint32_t), s));
    a.parent = parent.p;
    a.root = root.p;
    a.best = best.p;
    a.cmax = cmax.p;
    a.ckey = ckey.p;
    a.edges = edges.p;
    a.n_edges = n_edges.p;
    const dim3 row_grid((uint32_t)((rows + kRunBlock - 1) / kRunBlock)), blk(kRunBlock);
    const dim3 act_grid((a.n_active + kRunBlock - 1) / kRunBlock);
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    hipLaunchKernelGGL(k_tree_init, row_grid, blk, 0, s, a);
    FS_TRY(clk.mark(1, s));
    FS_HIP(hipGetLastError());
    // A round that adds an edge at least halves the families that still have one: fewer rounds
    // than FS_TREE_MAX_ROUNDS for any number of works, and the loop does not rely on it.
    uint32_t total = 0;
    for (uint32_t round = 0; total + 1 < a.n_active; ++round) {
      if (round == FS_TREE_MAX_ROUNDS) {
        fs_set_error("tree: no forest after %u rounds over %u works", FS_TREE_MAX_ROUNDS,
                     a.n_active);
        return FS_E_DEVICE;
      }
      FS_TRY(clk.mark(2, s));
      hipLaunchKernelGGL(k_tree_flatten, row_grid, blk, 0, s, a);
      FS_TRY(clk.mark(3, s));
      hipLaunchKernelGGL(k_tree_best, dim3((uint32_t)blocks), dim3(kBlock), 0, s, a);
      FS_TRY(clk.mark(4, s));
      hipLaunchKernelGGL(k_tree_level, act_grid, blk, 0, s, a);
      hipLaunchKernelGGL(k_tree_choose, act_grid, blk, 0, s, a);
      FS_TRY(clk.mark(5, s));
      hipLaunchKernelGGL(k_tree_hook, act_grid, blk, 0, s, a);
      FS_TRY(clk.mark(6, s));
      FS_HIP(hipGetLastError());
      uint32_t now = 0;
      FS_HIP(hipMemcpyAsync(&now, n_edges.p, sizeof now, hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
      for (int k = 0; k < 4; ++k) t_ms[1 + k] += clk.elapsed(2 + k, 3 + k);
      if (now >= a.n_active) {
        fs_set_error("tree: %u edges over %u works", now, a.n_active);
        return FS_E_DEVICE;
      }
      if (now == total) break;
      total = now;
      t_ms[8] += 1.0;
    }
    std::vector<uint4> h_edges(2 * (size_t)total);
    std::vector<uint32_t> h_work_of(a.n_active), h_covered(a.n_active);
    if (total) {
      FS_TRY(clk.mark(2, s));
      hipLaunchKernelGGL(k_tree_detail, dim3((total + kRunBlock - 1) / kRunBlock), blk, 0, s, a,
                         total);
      FS_TRY(clk.mark(3, s));
      FS_HIP(hipGetLastError());
      FS_HIP(hipMemcpyAsync(h_edges.data(), edges.p, h_edges.size() * sizeof(uint4),
                            hipMemcpyDeviceToHost, s));
    }
    FS_HIP(hipMemcpyAsync(h_work_of.data(), cj.work_of.p, a.n_active * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, s));
    FS_HIP(hipMemcpyAsync(h_covered.data(), cj.covered.p, a.n_active * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    t_ms[0] = clk.elapsed(0, 1);
    if (total) t_ms[5] = clk.elapsed(2, 3);
    const auto t1 = std::chrono::steady_clock::now();
    FS_TRY(out.run(n_works, a.n_active, h_work_of, h_covered, h_edges));
    t_ms[6] = host_ms(t1);
    t_ms[7] = host_ms(t0);
    return FS_OK;
  }
};

// the rules both entry points share
int tree_check(uint64_t n_rows, uint32_t n_works, uint32_t n_script, uint32_t min_words,
               uint32_t measure, uint32_t min_shared, uint32_t min_level, const void* works,
               const void* merges, uint64_t cap_merges, uint64_t* n_merges, const void* levels,
               uint64_t cap_levels, uint64_t* n_levels) {
  if (!n_merges || !n_levels || (n_works && !works) || (cap_merges && !merges) ||
      (cap_levels && !levels)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_shared == 0) {
    fs_set_error("min_words and min_shared must be at least 1");
    return FS_E_INVALID;
  }
  if (measure != FS_TREE_JACCARD && measure != FS_TREE_SHARED) {
    fs_set_error("measure %u: FS_TREE_JACCARD or FS_TREE_SHARED", measure);
    return FS_E_INVALID;
  }
  if (measure == FS_TREE_JACCARD && min_level > 1000000u) {
    fs_set_error("min_level %u: a Jaccard level is in parts per million", min_level);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("trees", n_rows, n_script));
  *n_merges = *n_levels = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_tree(int device, const uint32_t* work, const uint32_t* fan_ix,
                       const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                       uint32_t n_script, uint32_t min_words, uint32_t max_gap, uint32_t measure,
                       uint32_t min_shared, uint32_t min_level, fs_tree_work* works,
                       fs_tree_merge* merges, uint64_t cap_merges, uint64_t* n_merges,
                       fs_tree_level* levels, uint64_t cap_levels, uint64_t* n_levels) {
  FS_TRY(tree_check(n_rows, n_works, n_script, min_words, measure, min_shared, min_level, works,
                    merges, cap_merges, n_merges, levels, cap_levels, n_levels));
  TreeJob job;
  if (!n_rows) {
    for (double& t : t_ms) t = 0.0;
    job.out.none(n_works);
  } else {
    if (!work || !fan_ix || !orig_ix) {
      fs_set_error("null argument");
      return FS_E_INVALID;
    }
    FS_ENTER(device);
    DBuf<fs_row> rows;
    FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, (uint32_t)n_rows));
    FS_TRY(job.run(rows.p, (uint32_t)n_rows, n_works, n_script, min_words, max_gap, measure,
                   min_shared, min_level, nullptr));
    FS_HIP(hipDeviceSynchronize());
  }
  const Replay& out = job.out;
  std::copy(out.works.begin(), out.works.end(), works);
  *n_merges = out.merges.size();
  *n_levels = out.levels.size();
  if (out.merges.size() > cap_merges || out.levels.size() > cap_levels) return FS_E_CAPACITY;
  std::copy(out.merges.begin(), out.merges.end(), merges);
  std::copy(out.levels.begin(), out.levels.end(), levels);
  return FS_OK;
}

extern "C" int fs_tree_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows, uint32_t n_works,
                            uint32_t min_words, uint32_t max_gap, uint32_t measure,
                            uint32_t min_shared, uint32_t min_level, fs_tree_work* d_works,
                            fs_tree_merge* d_merges, uint64_t cap_merges, uint64_t* n_merges,
                            fs_tree_level* d_levels, uint64_t cap_levels, uint64_t* n_levels) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: trees take up to %u", (unsigned long long)ix->n_script,
                 FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(tree_check(n_rows, n_works, (uint32_t)ix->n_script, min_words, measure, min_shared,
                    min_level, d_works, d_merges, cap_merges, n_merges, d_levels, cap_levels,
                    n_levels));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_works & 15) ||
      ((uintptr_t)d_merges & 15) || ((uintptr_t)d_levels & 15)) {
    fs_set_error("d_rows, d_works, d_merges and d_levels must be 16-byte aligned device "
                 "pointers");
    return FS_E_INVALID;
  }
  FS_ENTER(ix->device);
  TreeJob job;
  FS_TRY(job.run(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                 measure, min_shared, min_level, ix->stream));
  const Replay& out = job.out;
  hipStream_t s = ix->stream;
  if (n_works)
    FS_HIP(hipMemcpyAsync(d_works, out.works.data(), n_works * sizeof(fs_tree_work),
                          hipMemcpyHostToDevice, s));
  *n_merges = out.merges.size();
  *n_levels = out.levels.size();
  const bool fits = out.merges.size() <= cap_merges && out.levels.size() <= cap_levels;
  if (fits && !out.merges.empty()) {
    FS_HIP(hipMemcpyAsync(d_merges, out.merges.data(), out.merges.size() * sizeof(fs_tree_merge),
                          hipMemcpyHostToDevice, s));
    FS_HIP(hipMemcpyAsync(d_levels, out.levels.data(), out.levels.size() * sizeof(fs_tree_level),
                          hipMemcpyHostToDevice, s));
  }
  FS_HIP(hipStreamSynchronize(s));
  return fits ? FS_OK : FS_E_CAPACITY;
}

extern "C" int fs_tree_times(double* ms) {
  return times_out(ms, t_ms, 9);
}
