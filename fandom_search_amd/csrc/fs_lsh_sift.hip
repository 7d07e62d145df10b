// fs_lsh_sift.hip -- between the prefilter and the per-window work, where one slot at most
// may differ (by vector ids, or by component ids) and no OOV id is involved.
//   k_lsh_sift     one lane per flagged window of k_expand's list: wildcard-key filter test,
//                  the n-gram's record of this string table (k_lsh_gramtab), the exact
//                  one-slot map; what is left goes onto the pending list
//   k_lsh_sift2    behind k_near_sift (fs_scan.hip), which has applied the filter already:
//                  numbers its lists' survivors and takes the same second stage
#include "fs_lsh.h"

using namespace fsdev;

namespace {

// Is script window s, which has the ids of fan window f in every slot but k, within the
// threshold?  The canonical distance of window_distance with n - 1 slots known to add q(v_t);
// true also when the premise does not hold in a way that cannot be decided here (the caller
// then takes the full path).  A key collision (other slots differ) is not a neighbour.
template <int NW>
__device__ __forceinline__ bool one_slot_within(const LshDev& L, uint32_t s, int k, const Ids16& f) {
  Ids16 u;
  load_ids(L.stok + s, L.n, &u);
  uint32_t uk = 0, fk = 0;
  bool agree = true;
#pragma unroll
  for (int t = 0; t < NW; ++t)
    if (t < L.n) {
      if (t == k) { uk = u.v[t]; fk = f.v[t]; }
      else agree = agree && u.v[t] == f.v[t];
    }
  if (!agree) return false;
  if (uk == fk) return true;
  double q[NW];
#pragma unroll
  for (int t = 0; t < NW; ++t)
    if (t < L.n) q[t] = L.q[f.v[t]];
  const double g = g_of(L, uk, fk);
  const fs_swin sw = L.sw[s];
  double ff = 0.0, sf = 0.0;
#pragma unroll
  for (int t = 0; t < NW; ++t)
    if (t < L.n) {
      ff = __dadd_rn(ff, q[t]);
      sf = __dadd_rn(sf, t == k ? g : q[t]);
    }
  const double d = __dsub_rn(1.0, __ddiv_rn(sf, __dmul_rn(sw.rss, __dsqrt_rn(ff))));
  return !(d == d) || d < L.thr;
}

// One lane per candidate, in front of k_lsh_verify: most candidates end here.
//   cg[i] = FS_NONE      no neighbour within the threshold
//   cg[i] = 0            a record: cbest[i], cw[i] (the record of its n-gram, k_lsh_gramtab)
//   cg[i] = FS_PENDING   k_lsh_verify works the window out, a wave at a time
// A kernel of its own: k_lsh_verify carries the scratch arrays and registers of the neighbour
// lists and the Levenshtein code, which these steps do not need; consecutive candidates sit
// in consecutive lanes, so the per-candidate arrays move in whole cache lines.
// The one-slot-wildcard keys of the window at `p` (made of the vector ids, or of the
// component ids: L.wild_tok): terms and fold for the caller, true when one of the n keys is in
// the grouped filter (three 16-byte blocks, requested together).
template <int NW>
__device__ __forceinline__ bool sift_keys(const CorpusDev& c, const LshDev& L, uint64_t p,
                                          uint32_t* term, uint32_t* fold_out, bool probe) {
  Ids16 kf;
  load_ids((L.wild_tok ? L.wild_tok : c.tok) + p, L.n, &kf);
  uint32_t fold = 0, gfold[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    term[k] = 0;
    if (k < L.n) {
      term[k] = fs_rotl(fs_premix(kf.v[k]), fs_rot_of(L.n - 1 - k));
      fold ^= term[k];
      gfold[fs_wild_group(k, L.n)] ^= term[k];
    }
  }
  *fold_out = fold;
  if (!probe) return true;
  const uint4* wb = reinterpret_cast<const uint4*>(L.wild);
  uint4 blk[3];
#pragma unroll
  for (int X = 0; X < 3; ++X) blk[X] = wb[fs_wild_block(fold ^ gfold[X], X, L.log2_wild)];
  bool pass = false;
#pragma unroll
  for (int k = 0; k < NW; ++k)
    if (k < L.n) {
      const uint32_t h = fs_wild_fkey(fold, term[k], k);
      const int X = fs_wild_group(k, L.n);
      const uint4 q = X == 0 ? blk[0] : X == 1 ? blk[1] : blk[2];
      pass = pass || ((q.x >> fs_wild_fbit(h, 0)) & (q.y >> fs_wild_fbit(h, 1)) &
                      (q.z >> fs_wild_fbit(h, 2)) & (q.w >> fs_wild_fbit(h, 3)) & 1u);
    }
  return pass;
}

// One lane per candidate, in two stages.  Stage 1, every candidate: the wildcard-key filter
// (one level of loads behind the candidate's position and ids).  Most candidates end there --
// 88 % at n = 8, 84 % over component ids -- and the deeper steps (exact table, one-slot map:
// five to eight more levels of dependent loads) ran at a tenth of the lanes while every wave
// had a survivor to wait for.  So the survivors queue up in LDS and stage 2 takes them 256 at
// a time, a full lane each (round 4: 90 -> 40 us per C2 batch at n = 8).
// k_lsh_sift's second stage for one candidate per thread (il = FS_NONE: none; every thread of
// the workgroup calls it: it holds barriers): the per-n-gram record, the exact one-slot map, or
// onto the pending list.  Shared by k_lsh_sift and k_lsh_sift2.
struct SiftOut {
  uint32_t* cg; uint32_t* cw; fs_best* cbest;
  const unsigned long long* tab_best; const uint32_t* tab_cnt;
  uint32_t* pend; uint32_t* pend_cnt;
  uint32_t* s_pn; uint32_t* s_pbase;          // LDS words of the workgroup
};
// CNT: with the counters of fs_index_lsh_counts (a form of its own: the kernels without them keep
// their registers)
template <int NW, bool WMAP, bool CNT>
__device__ __forceinline__ void sift_stage2(const CorpusDev& c, const LshDev& L, const GramIndexDev& g,
                                            const SiftOut& o, uint32_t il, uint64_t p_in, uint32_t* matches_io) {
  const int lane = threadIdx.x & 63;
  uint32_t* const cg = o.cg; uint32_t* const cw = o.cw; fs_best* const cbest = o.cbest;
  const unsigned long long* const tab_best = o.tab_best; const uint32_t* const tab_cnt = o.tab_cnt;
  uint32_t* const pend = o.pend; uint32_t* const pend_cnt = o.pend_cnt;
  uint32_t& s_pn = *o.s_pn; uint32_t& s_pbase = *o.s_pbase;
  uint32_t& matches = *matches_io;
  bool live = il != FS_NONE;
  // 2. A window with the ids of a script n-gram (and the strings of those ids) takes the
  //    n-gram's record of this string table (k_lsh_gramtab): no bucket is walked for it.
  uint32_t gram = FS_NONE;
  const uint64_t p = live ? p_in : 0;
  if (tab_cnt && live && !(L.diag & 128)) {
    uint32_t w = 0, kept = 0;
    gram = verify_window(c, g, p, &w, &kept);
    if (gram != FS_NONE) {
      const uint32_t have = tab_cnt[gram];
      if (have == 1) {
        cg[il] = FS_NONE;                             // (no neighbour within the threshold)
      } else {
        const uint4* m = reinterpret_cast<const uint4*>(tab_best + 4 * (size_t)gram);
        uint4* dst = reinterpret_cast<uint4*>(&cbest[il]);
        dst[0] = m[0]; dst[1] = m[1];
        cg[il] = 0;
        cw[il] = w;
        matches += have - 1;
      }
      if (CNT) {                                      // diagnostics (fs_index_lsh_counts)
        lsh_count(L.lsh_cnt, kCntRecordNeighbours, have != 1);
        lsh_count(L.lsh_cnt, kCntRecordAlone, have == 1);
      }
      live = false;
    }
  }
  // 3. Not a script n-gram itself: enumerate the script n-grams that equal the window in all
  //    slots but one (every neighbour within the threshold is one of them: m_min = n - 1) and
  //    take their canonical distances.  None within the threshold: whatever the buckets hold,
  //    nothing survives the threshold, and the window needs no LSH work.  One 32-byte bucket
  //    of the map per slot, all n requested together; a window with more than two such
  //    n-grams, or a full bucket in its way, is left to k_lsh_verify.
  if (WMAP && live && L.wild && p + L.n <= c.n_tok && !(L.diag & 256)) {
    uint32_t term[NW], fold = 0;
    sift_keys<NW>(c, L, p, term, &fold, false);
    Ids16 f;
    load_ids(c.tok + p, L.n, &f);
    uint32_t s0 = 0, s1 = 0, nh = 0;
    int k0 = 0, k1 = 0;
    bool possible = false;
#pragma unroll
    for (int k = 0; k < NW; ++k)
      if (k < L.n) {
        const uint32_t h = fs_wild_key(fold, term[k], k);
        const uint4* bp = reinterpret_cast<const uint4*>(L.wmap + 4 * (size_t)fs_wmap_slot(h, L.log2_wmap));
        const uint4 a = bp[0], b = bp[1];
        const uint32_t key[4] = {a.x, a.z, b.x, b.z}, val[4] = {a.y, a.w, b.y, b.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (val[e] && key[e] == h) {
            if (nh == 0) { s0 = val[e] - 1; k0 = k; }
            else if (nh == 1) { s1 = val[e] - 1; k1 = k; }
            ++nh;
          }
        possible = possible || val[3] != 0;       // (filled in order: the bucket is full)
      }
    const bool full = possible;
    possible = possible || nh > 2;
    if (L.diag & 512) possible = possible || nh > 0;                 // diagnostics: no distances here
    if (!possible && nh > 0) possible = one_slot_within<NW>(L, s0, k0, f);
    if (!possible && nh > 1) possible = one_slot_within<NW>(L, s1, k1, f);
    if (!possible) { cg[il] = FS_NONE; live = false; }
    if (CNT) {                                                       // diagnostics (fs_index_lsh_counts)
      lsh_count(L.lsh_cnt, kCntWmapPendingFull, full);
      lsh_count(L.lsh_cnt, kCntWmapPendingMany, !full && nh > 2);
      lsh_count(L.lsh_cnt, kCntWmapPendingDistance, !full && nh <= 2 && possible);
      lsh_count(L.lsh_cnt, kCntWmapEnded0, !possible && nh == 0);
      lsh_count(L.lsh_cnt, kCntWmapEnded1, !possible && nh == 1);
      lsh_count(L.lsh_cnt, kCntWmapEnded2, !possible && nh == 2);
    }
  }
  // what is left: onto the list k_lsh_verify deals out window by window (pending windows
  // come in runs, the boundary windows of one quoted passage, so dealing out blocks of
  // candidates leaves a few waves with most of the work)
  // (one addition to the list's counter per workgroup: five thousand waves adding to the one
  // address took 5 ns each, a third of the kernel)
  const uint64_t pb = __ballot(live);
  uint32_t wbase = 0;
  if (pb && lane == 0) wbase = atomicAdd(&s_pn, (uint32_t)__popcll(pb));      // LDS
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n_p = s_pn;
    s_pbase = n_p ? atomicAdd(pend_cnt, n_p) : 0u;
    s_pn = 0;
  }
  __syncthreads();
  if (live) {
    const uint32_t base = s_pbase + (uint32_t)__builtin_amdgcn_readlane((int)wbase, 0);
    cg[il] = FS_PENDING;
    pend[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(pb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pb, 0u))] = (uint32_t)il;
  }
}

template <int NW, bool WMAP, int NN, bool CNT>
__global__ __launch_bounds__(256, 5) void k_lsh_sift(CorpusDev c, LshDev L, GramIndexDev g,
                                                  const uint32_t* __restrict__ cpos, NSrc nc,
                                                  uint32_t* __restrict__ cg, uint32_t* __restrict__ cw,
                                                  fs_best* __restrict__ cbest,
                                                  uint32_t* __restrict__ bmatch,
                                                  const unsigned long long* __restrict__ tab_best,
                                                  const uint32_t* __restrict__ tab_cnt,
                                                  uint32_t* __restrict__ pend,
                                                  uint32_t* __restrict__ pend_cnt) {
  __shared__ uint32_t s_w32[4];
  __shared__ uint32_t s_q[1024];         // survivors of stage 1 (candidate numbers): at most 255 + 3 * 256
  __shared__ uint32_t s_qn, s_pn, s_pbase;
  const uint32_t total = nc.get();
  const int lane = threadIdx.x & 63;
  uint32_t matches = 0;
  if (L.diag & 8192) {                         // diagnostics: the launch by itself
    if (threadIdx.x == 0) bmatch[blockIdx.x] = 0;
    return;
  }
  if (threadIdx.x == 0) { s_qn = 0; s_pn = 0; }
  __syncthreads();
  // stage 2 for one queued candidate (FS_NONE: none); every thread of the workgroup calls it
  const SiftOut so{cg, cw, cbest, tab_best, tab_cnt, pend, pend_cnt, &s_pn, &s_pbase};
  auto stage2 = [&](uint32_t il) {
    sift_stage2<NW, WMAP, CNT>(c, L, g, so, il, il != FS_NONE ? (uint64_t)cpos[il] : 0ull, &matches);
  };
  // U candidates per lane and pass, their loads level by level: positions, ids, filter blocks
  constexpr int U = NW <= 8 ? 3 : 2;
  const uint64_t pass = (uint64_t)gridDim.x * 256;
  for (uint64_t i0 = (uint64_t)blockIdx.x * 256; i0 < total; i0 += pass * U) {
    uint64_t il[U], p[U];
    bool live[U], probe[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      il[u] = i0 + (uint64_t)u * pass + threadIdx.x;
      live[u] = il[u] < total;
      p[u] = (L.wild && live[u]) ? cpos[il[u]] : 0;
    }
    // 1. (no OOV anywhere, at most one slot may differ) a window none of whose n one-slot-
    //    wildcard keys is a script window's key has no neighbour within the threshold
    if (L.wild) {
      uint32_t kf[U][NW];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        probe[u] = live[u] && p[u] + L.n <= c.n_tok;
        if (L.diag & 4096) { if (live[u]) cg[il[u]] = FS_NONE; live[u] = false; probe[u] = false; }   // diagnostics
        // (the window start is only 4-byte aligned; the buffers are padded: fs_device.h, load_ids)
        const uint4* src = reinterpret_cast<const uint4*>((L.wild_tok ? L.wild_tok : c.tok) + (probe[u] ? p[u] : 0));
#pragma unroll
        for (int q4 = 0; q4 < NW / 4; ++q4) {
          uint4 t = make_uint4(0, 0, 0, 0);
          if (q4 < 2 || L.n > 8) t = src[q4];
          kf[u][4 * q4] = t.x; kf[u][4 * q4 + 1] = t.y; kf[u][4 * q4 + 2] = t.z; kf[u][4 * q4 + 3] = t.w;
        }
      }
      const uint4* wb = reinterpret_cast<const uint4*>(L.wild);
      uint4 blk0[U], blk1[U], blk2[U];
      uint32_t fold[U];
      const int n = NN ? NN : L.n;              // (NN: the window size at compile time -- groups and rotations are constants then)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint32_t g0 = 0, g1 = 0, g2 = 0;
        fold[u] = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k)
          if (k < n) {
            const uint32_t t = fs_rotl(fs_premix(kf[u][k]), fs_rot_of(n - 1 - k));
            const int X = fs_wild_group(k, n);
            fold[u] ^= t;
            g0 ^= X == 0 ? t : 0u; g1 ^= X == 1 ? t : 0u; g2 ^= X == 2 ? t : 0u;
          }
        if (L.diag & 2048) { g0 = g1 = g2 = fold[u] ^ (uint32_t)threadIdx.x; }    // diagnostics: the same blocks for every wave
        blk0[u] = wb[fs_wild_block(fold[u] ^ g0, 0, L.log2_wild)];
        blk1[u] = wb[fs_wild_block(fold[u] ^ g1, 1, L.log2_wild)];
        blk2[u] = wb[fs_wild_block(fold[u] ^ g2, 2, L.log2_wild)];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        uint32_t any = 0;                       // bit 0: one of the keys is in the filter
#pragma unroll
        for (int k = 0; k < NW; ++k)
          if (k < n) {
            const uint32_t t = fs_rotl(fs_premix(kf[u][k]), fs_rot_of(n - 1 - k));
            const uint32_t h = fs_wild_fkey(fold[u], t, k);
            const int X = fs_wild_group(k, n);
            uint4 q;
            q.x = X == 0 ? blk0[u].x : X == 1 ? blk1[u].x : blk2[u].x;
            q.y = X == 0 ? blk0[u].y : X == 1 ? blk1[u].y : blk2[u].y;
            q.z = X == 0 ? blk0[u].z : X == 1 ? blk1[u].z : blk2[u].z;
            q.w = X == 0 ? blk0[u].w : X == 1 ? blk1[u].w : blk2[u].w;
            any |= shr_by_byte<0>(q.x, h) & shr_by_byte<1>(q.y, h) & shr_by_byte<2>(q.z, h) & shr_by_byte<3>(q.w, h);
          }
        bool pass1 = (any & 1u) != 0;
        if (L.diag & 1024) pass1 = false;                                          // diagnostics: nothing survives
        if (probe[u] && !pass1) { cg[il[u]] = FS_NONE; live[u] = false; }
      }
    }
    // the survivors onto the queue (a slot per wave's worth of them).  The barrier keeps a
    // fast wave's additions to s_qn behind every wave's read of it at the end of the round
    // before (the read decides a workgroup-uniform branch around barriers)
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint64_t sb = __ballot(live[u]);
      uint32_t base = 0;
      if (sb) {
        const int leader = __ffsll((unsigned long long)sb) - 1;
        if (lane == leader) base = atomicAdd(&s_qn, (uint32_t)__popcll(sb));
        base = (uint32_t)__builtin_amdgcn_readlane((int)base, leader);
        if (live[u])
          s_q[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(sb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)sb, 0u))] = (uint32_t)il[u];
      }
    }
    __syncthreads();
    // stage 2 once 256 are queued, all of them at the end
    const bool last = i0 + pass * U >= total;
    uint32_t qn = s_qn;
    while (qn >= 256 || (last && qn > 0)) {
      const uint32_t take = qn < 256 ? qn : 256u;
      const uint32_t mine = threadIdx.x < take ? s_q[qn - take + threadIdx.x] : FS_NONE;
      __syncthreads();
      if (threadIdx.x == 0) s_qn = qn - take;
      stage2(mine);
      __syncthreads();
      qn = s_qn;
    }
  }
  uint32_t tot;
  block_excl_scan(matches, s_w32, &tot);
  if (threadIdx.x == 0) {
    bmatch[blockIdx.x] = tot;
    // (the sums are read kNB at a time: the workgroups that were not launched have none)
    for (uint32_t b = blockIdx.x + gridDim.x; b < (uint32_t)kNB; b += gridDim.x) bmatch[b] = 0;
  }
}

// k_lsh_sift2 (round 5): behind k_near_sift, which has put the candidates that pass the wildcard
// filter into one list per wave range.  Numbers them across the ranges (chunk sums: four ranges
// a chunk), writes the flat arrays the kernels behind expect -- an eighth of the entries
// k_expand used to make -- and takes k_lsh_sift's second stage for each.  Every workgroup takes
// an equal share of the numbered survivors (its place among the chunks by a search in the
// chunk sums' prefix, which each workgroup makes for itself in LDS): one pass of full waves.
// (A workgroup per chunk measured 45 us at n = 8 and 67 at n = 10: a C2 batch leaves 70 to 100
// survivors per chunk, so the deep steps ran at a third of the lanes, twice over.)
template <int NW, bool WMAP, bool CNT>
__global__ __launch_bounds__(256, 5) void k_lsh_sift2(CorpusDev c, LshDev L, GramIndexDev g,
                                                   const uint32_t* __restrict__ slist, uint32_t caps,
                                                   const uint32_t* __restrict__ scount,
                                                   const uint32_t* __restrict__ bsum,
                                                   uint32_t* __restrict__ cpos, uint32_t ccap,
                                                   uint32_t* __restrict__ cg, uint32_t* __restrict__ cw,
                                                   fs_best* __restrict__ cbest,
                                                   uint32_t* __restrict__ bmatch,
                                                   const unsigned long long* __restrict__ tab_best,
                                                   const uint32_t* __restrict__ tab_cnt,
                                                   uint32_t* __restrict__ pend, fs_status* st) {
  static_assert(kNB == 8 * 256, "eight chunk sums per thread");
  __shared__ uint32_t s_w32[4];
  __shared__ uint32_t s_pn, s_pbase;
  __shared__ uint32_t s_pre[kNB + 1];                 // survivors in front of chunk i
  uint32_t matches = 0;
  if (threadIdx.x == 0) s_pn = 0;
  {
    uint32_t v[8], sum = 0;
    const uint4* src = reinterpret_cast<const uint4*>(bsum + 8 * threadIdx.x);
    const uint4 a = src[0], b = src[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += v[k];
    uint32_t tot_all;
    uint32_t run = block_excl_scan(sum, s_w32, &tot_all);
#pragma unroll
    for (int k = 0; k < 8; ++k) { s_pre[8 * threadIdx.x + k] = run; run += v[k]; }
    if (threadIdx.x == 0) s_pre[kNB] = tot_all;
  }
  __syncthreads();
  const uint32_t total = s_pre[kNB];
  const SiftOut so{cg, cw, cbest, tab_best, tab_cnt, pend, &st->lsh_pending, &s_pn, &s_pbase};
  // this workgroup's share, in whole steps of 256
  const uint32_t steps = (total + 255) / 256;
  const uint32_t per = (steps + gridDim.x - 1) / gridDim.x;
  const uint32_t lo = (uint32_t)min((uint64_t)blockIdx.x * per * 256, (uint64_t)total);
  const uint32_t hi = (uint32_t)min((uint64_t)(blockIdx.x + 1) * per * 256, (uint64_t)total);
  for (uint32_t t0 = lo; t0 < hi; t0 += 256) {        // (workgroup-uniform)
    const uint32_t il = t0 + threadIdx.x;
    bool live = il < hi && il < ccap;                 // (beyond the arrays: n_cands says so, the search is repeated)
    uint32_t p = 0;
    if (live) {
      uint32_t a = 0, b = kNB;                        // the last chunk with s_pre[chunk] <= il
      while (b - a > 1) {
        const uint32_t mid = (a + b) >> 1;
        if (s_pre[mid] <= il) a = mid; else b = mid;
      }
      uint32_t off = il - s_pre[a];
      const uint4 cn = *reinterpret_cast<const uint4*>(scount + 4 * a);
      const uint32_t c0 = min(cn.x, caps), c1 = min(cn.y, caps), c2 = min(cn.z, caps);
      uint32_t r = 0;
      if (off >= c0) { off -= c0; r = 1; if (off >= c1) { off -= c1; r = 2; if (off >= c2) { off -= c2; r = 3; } } }
      p = slist[(size_t)(4 * a + r) * caps + off];
      cpos[il] = p;
    }
    sift_stage2<NW, WMAP, CNT>(c, L, g, so, live ? il : FS_NONE, p, &matches);
  }
  if (blockIdx.x == 0) {                              // for the kernels behind and the host
    uint32_t over = 0;
    for (uint32_t i = threadIdx.x; i < 4u * kNB; i += 256) over = max(over, scount[i]);
    if (threadIdx.x == 0) st->n_cands = total;
    if (over > caps) atomicMax(&st->max_recs, over);  // a range's list was too short (rare: the search is repeated)
  }
  uint32_t tot;
  block_excl_scan(matches, s_w32, &tot);
  if (threadIdx.x == 0) {
    bmatch[blockIdx.x] = tot;
    for (uint32_t b = blockIdx.x + gridDim.x; b < (uint32_t)kNB; b += gridDim.x) bmatch[b] = 0;
  }
}

// the kernels for this index: its window size, with or without the exact one-slot map, with the
// counters where the index has them
template <bool CNT>
auto sift_kernel(const LshDev& L) -> decltype(&k_lsh_sift<8, true, 0, CNT>) {
  auto sift = L.n <= 8 ? (L.wmap ? k_lsh_sift<8, true, 0, CNT> : k_lsh_sift<8, false, 0, CNT>)
                       : (L.wmap ? k_lsh_sift<FS_MAX_WINDOW, true, 0, CNT> : k_lsh_sift<FS_MAX_WINDOW, false, 0, CNT>);
  switch (L.n) {            // the common window sizes with their size at compile time
    case 6: sift = L.wmap ? k_lsh_sift<8, true, 6, CNT> : k_lsh_sift<8, false, 6, CNT>; break;
    case 8: sift = L.wmap ? k_lsh_sift<8, true, 8, CNT> : k_lsh_sift<8, false, 8, CNT>; break;
    case 10: sift = L.wmap ? k_lsh_sift<FS_MAX_WINDOW, true, 10, CNT> : k_lsh_sift<FS_MAX_WINDOW, false, 10, CNT>; break;
    default: break;
  }
  return sift;
}
template <bool CNT>
auto sift2_kernel(const LshDev& L) -> decltype(&k_lsh_sift2<8, true, CNT>) {
  return L.n <= 8 ? (L.wmap ? k_lsh_sift2<8, true, CNT> : k_lsh_sift2<8, false, CNT>)
                  : (L.wmap ? k_lsh_sift2<FS_MAX_WINDOW, true, CNT> : k_lsh_sift2<FS_MAX_WINDOW, false, CNT>);
}

}  // namespace

// near: the candidates come from k_near_sift's lists (the wildcard filter applied):
// k_lsh_sift2 numbers them and takes the second stage, instead of k_lsh_sift over k_expand's list
int lsh_launch_sift(fs_index* ix, fs_corpus* c, const LshDev& L, uint32_t ccap, hipStream_t s,
                    const fs_near_lists* near) {
  fs_status* st = ix->cur->d_status.p;
  const NSrc nc{&st->n_cands, 1, ccap, 0};
  // per-n-gram records of this string table (k_lsh_gramtab, fs_corpus_update_end)
  const unsigned long long* tab_best = nullptr;
  const uint32_t* tab_cnt = nullptr;
  if (c->gramtab_ready && !c->has_str && !c->has_oov) {
    tab_best = c->d_gramtab_best.p;
    tab_cnt = c->d_gramtab_cnt.p;
  }
  const auto sift = L.lsh_cnt ? sift_kernel<true>(L) : sift_kernel<false>(L);
  if (near) {
    const auto sift2 = L.lsh_cnt ? sift2_kernel<true>(L) : sift2_kernel<false>(L);
    const uint32_t blocks = lsh_resident_blocks(ix, reinterpret_cast<const void*>(sift2));
    hipLaunchKernelGGL(sift2, dim3(blocks), dim3(256), 0, s, c->dev(), L, ix->gram_dev(),
                       near->slist, near->caps, near->scount, ix->cur->w_bsum.p,
                       ix->cur->w_cpos.p, ccap, ix->cur->w_cg.p, ix->cur->w_cw.p, ix->cur->w_cbest.p,
                       ix->cur->w_bsum.p + kNB, tab_best, tab_cnt, ix->cur->w_pend.p, st);
    if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_sift2");
  } else {
  const uint32_t sift_blocks = lsh_resident_blocks(ix, reinterpret_cast<const void*>(sift));
  hipLaunchKernelGGL(sift, dim3(sift_blocks), dim3(256), 0, s, c->dev(), L, ix->gram_dev(),
                     ix->cur->w_cpos.p, nc, ix->cur->w_cg.p, ix->cur->w_cw.p,
                     ix->cur->w_cbest.p, ix->cur->w_bsum.p + kNB, tab_best, tab_cnt, ix->cur->w_pend.p,
                     &st->lsh_pending);
    if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_sift");
  }
  return FS_OK;
}
