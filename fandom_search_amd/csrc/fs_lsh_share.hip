// fs_lsh_share.hip -- the first kernel of a general search: which fan windows have a script
// window within the threshold (fs_launch_lsh_scan picks among the three).
//   k_lsh_scan     one block per 256-window sub-tile: keys for all 256 windows
//                  (threads = projection columns, coalesced reads of A rows), then
//                  the (window, bucket candidate) pairs of the sub-tile are dealt out
//                  evenly over the threads and each asks "within the threshold?"; the
//                  per-window answers go out in the scan's bitmap format, so k_expand /
//                  k_rows of fs_post.hip are shared
//   k_share_gate   in front of k_lsh_scan on tables whose vectors are not unit length: the
//                  windows that need keys at all ("the share rule" below)
//   k_share_scan   in k_lsh_scan's place on such tables: the windows that can have a script window
//                  within the threshold at all, by the shares of the squared norms their agreeing
//                  slots hold, then the script windows behind their subset keys one by one
#include "fs_lsh.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

using namespace fsdev;

namespace {

// ---- the share rule ----------------------------------------------------------------
//
// For tables whose vectors are not unit length none of the integer prefilters applies ("at most
// one slot may differ" is false there: a window's squared norm may sit in a few slots, and the
// others may then hold anything).  What holds for any norms: call two vectors *near* when their
// cosine exceeds gamma (components of that relation over the table: compa; a vector of norm 0 is
// near nothing), let D be the slots of a window pair (F, S) whose vectors lie in different
// components, and A, B the shares of |F|^2 and |S|^2 those slots hold.  Then, slot by slot
// dot(f_k, s_k) <= |f_k||s_k| and <= gamma |f_k||s_k| on D, and by Cauchy-Schwarz on either group
//   cos(F, S) <= sqrt((1 - A)(1 - B)) + gamma sqrt(A B)  <=  sqrt(1 - A (1 - gamma^2)),
// so a pair within the threshold (cos > tau = 1 - thr - 1e-6) has A < phi and B < phi,
// phi = (1 - tau^2) / (1 - gamma^2): the slots that agree in their components hold more than
// 1 - phi of either window's squared norm.  Two sound skips come of it, both in k_lsh_scan:
//   * the gate, per fan window: the subsets M of slots that are *heavy* (hold that share of the
//     fan window) and minimal (no slot can go) are asked for in a filter that holds, for every
//     script window, the key (slots, component ids there) of every subset of its slots.  The set
//     of agreeing slots of a pair within the threshold is heavy, so it contains a minimal heavy
//     subset, and that one's key is in the filter: a window none of whose keys is there has no
//     script window within the threshold, needs no LSH keys and walks no bucket.  (FS_LSH_SHARE
//     bit 2: the filter holds the script windows' own heavy subsets only and every heavy subset
//     of the fan window is asked for -- the agreeing set is heavy on both sides.)  Squared norms
//     are integers here (floor(q * share_scale)), so "heavy" is one exact comparison however the
//     subset is summed, with the slack of the rounding on the permissive side.
//   * the test, per (fan window, bucket member): A from the fan side alone (LDS), then B and the
//     two-sided bound, in front of window_distance and its pair-table entries.
// An out-of-vocabulary fan token (at most three coordinates, all 1) is far from every script
// vector when sqrt(3) max_d |u_d| / |u| <= gamma for all of them (checked at index build);
// otherwise (share_flags bit 3) its slot counts as agreeing with anything.  Scripts with
// out-of-vocabulary tokens do not use the rule.
// Component id of a fan token under the share rule.  A table row: compa.  An out-of-vocabulary
// token is a vector of at most three ones: far from every table row of the script (checked at
// index build), and against the script's own out-of-vocabulary vectors, by the sets of hot
// positions -- equal sets are the same vector (cosine 1: that script vector's component), three
// distinct positions against another three share at most two (2/3: far, gamma >= 0.668 is
// required of such an index), and every other case involves a set of fewer than three (a hash
// that met itself): cosines 0.71 and 0.82 occur there, so a fan token with fewer than three
// distinct positions, or one that contains a two-position vector of the script, is FS_WILD: it
// counts as agreeing with anything.  (A script token with fewer than three positions has a
// component of its own that no fan token carries: fan tokens near it are all FS_WILD.)
__device__ __forceinline__ uint32_t share_oov_lookup(const LshDev& L, uint32_t key) {
  const uint32_t mask = (1u << L.log2_oovmap) - 1u;
  for (uint32_t at = fs_mix24(key) & mask;; at = (at + 1) & mask) {
    const uint2 e = L.oovmap[at];
    if (e.y == 0u) return 0u;                      // (values are stored + 1)
    if (e.x == key) return e.y;
  }
}
__device__ __forceinline__ uint32_t share_comp(const LshDev& L, uint32_t id) {
  if (!(id & FS_OOV_FLAG)) return L.compa[id];
  if (L.share_flags & 8) return FS_WILD;
  if (!L.oovmap || L.diag == 0x1000000) return FS_NONE;   // (diagnostics 0x1000000, a wrong rule on purpose: what tools/stress_share.py must catch)
  uint32_t x, y, z;
  oov_hot(id, L.D, &x, &y, &z);
  uint32_t t;
  if (x > y) { t = x; x = y; y = t; }
  if (y > z) { t = y; y = z; z = t; }
  if (x > y) { t = x; x = y; y = t; }
  if (x == y || y == z) return FS_WILD;
  const uint32_t D = (uint32_t)L.D;
  if (share_oov_lookup(L, 0x80000000u | (x * D + y)) || share_oov_lookup(L, 0x80000000u | (x * D + z)) ||
      share_oov_lookup(L, 0x80000000u | (y * D + z)))
    return FS_WILD;
  const uint32_t c = share_oov_lookup(L, (x * D + y) * D + z);
  return c ? c - 1u : FS_NONE;
}

// The keys a fan window asks for (its minimal heavy subsets; all heavy ones under share_flags bit 2),
// into list[j * 256]: their number, or -1 when the window is not constrained (the rule says nothing
// about it, or the list is too short for its keys).
// (the subsets of the slots K .. KEND - 1 depth first: a subset's sum and minimum are its parent's and
// one operation each; what leaves is the subset's mask, 16 bits -- its key is made by whoever reads
// the list, once per subset asked for instead of once per subset)
// (a subset of a window's slots: a byte for windows of up to eight slots)
template <int N> using share_mask_t = std::conditional_t<(N <= 8), uint8_t, uint16_t>;

template <int N, int K, int KEND, uint32_t M>
struct ShareSubsets {
  static __device__ __forceinline__ void go(const uint32_t (&qi)[N], uint32_t usable, int thr, bool every,
                                            uint32_t sum, uint32_t mn, share_mask_t<N>* list, int cap, int& cnt) {
    if constexpr (K == KEND) {
      if constexpr (M != 0u) {
        const bool ask = (M & ~usable) == 0u && (int)sum >= thr && (every || (int)(sum - mn) < thr);
        if (ask) {
          if (cnt < cap) list[cnt * 256] = (share_mask_t<N>)M;
          ++cnt;
        }
      }
    } else {
      ShareSubsets<N, K + 1, KEND, M>::go(qi, usable, thr, every, sum, mn, list, cap, cnt);
      ShareSubsets<N, K + 1, KEND, (M | (1u << K))>::go(qi, usable, thr, every, sum + qi[K], qi[K] < mn ? qi[K] : mn,
                                                        list, cap, cnt);
    }
  }
};

// Windows of more than six slots, run by run (fs_share_blocks): the agreeing slots of a pair within
// the threshold hold more than `lim` of the fan window's squared norm, so in at least one run they
// hold more than `lim` of *that run's* -- the run's minimal subsets that do are asked for, with
// the slots' own numbers in the key.  (A run the rule says nothing about -- all of it slots that
// agree with anything -- leaves the window unconstrained.)
template <int N, int R>
__device__ __forceinline__ bool share_asks_run(const LshDev& L, const uint32_t (&qi)[N], const uint32_t (&wild)[N],
                                               uint32_t usable, bool every, share_mask_t<N>* list, int cap, int& cnt) {
  constexpr int K0 = fs_share_block_start(N, R), K1 = fs_share_block_start(N, R + 1);
  uint32_t all = 0, base = 0;
#pragma unroll
  for (int k = K0; k < K1; ++k) { all += qi[k]; base += wild[k]; }
  // heavy(M): sum_M qi >= thr.  (With x = q * scale real and qi = floor(x): a truly heavy M has
  // sum_M x >= lim sum x - sum_O x, so sum_M qi > lim * all - base - (K1 - K0).)
  const int thr = (int)floorf(L.share_lim * (float)all) - (int)base - (K1 - K0) - 2;
  if (thr <= 0) return false;
  ShareSubsets<N, K0, K1, 0u>::go(qi, usable, thr, every, 0u, 0xFFFFFFFFu, list, cap, cnt);
  return true;
}

// The subsets a fan window asks for -- their slots as bit masks, into list[j * 256] --: their number,
// or -1 when the window is not constrained (the rule says nothing about it, or the list is too
// short).  The key of a subset is made where it is needed (share_key_of: from the slots' terms).
template <int N>
__device__ __forceinline__ int share_asks(const LshDev& L, const uint32_t* cmp, const double* qd,
                                          share_mask_t<N>* list, int cap) {
  uint32_t qi[N], wild[N];
  uint32_t usable = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    qi[k] = (uint32_t)(qd[k] * L.share_scale);
    const uint32_t c = cmp[k];
    wild[k] = c == FS_WILD ? qi[k] + 1 : 0u;
    usable |= c < FS_WILD ? 1u << k : 0u;
  }
  const bool every = (L.share_flags & 4) != 0;
  int cnt = 0;
  bool ok = share_asks_run<N, 0>(L, qi, wild, usable, every, list, cap, cnt);
  if constexpr (fs_share_blocks(N) > 1) ok = ok && share_asks_run<N, 1>(L, qi, wild, usable, every, list, cap, cnt);
  if constexpr (fs_share_blocks(N) > 2) ok = ok && share_asks_run<N, 2>(L, qi, wild, usable, every, list, cap, cnt);
  return !ok || cnt > cap ? -1 : cnt;
}

template <int N>
__device__ __forceinline__ void share_terms(const uint32_t* cmp, uint32_t (&t)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) t[k] = fs_share_term(cmp[k], k);   // (a slot without a component is in no subset)
}
template <int N>
__device__ __forceinline__ uint32_t share_key_of(const uint32_t (&t)[N], uint32_t m) {
  uint32_t fold = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) fold ^= ((m >> k) & 1u) ? t[k] : 0u;
  return fs_share_key(fold, m);
}

template <int N>
__device__ __forceinline__ bool share_gate(const LshDev& L, const uint32_t* cmp, const double* qd,
                                           share_mask_t<N>* list, int cap) {
  const int cnt = share_asks<N>(L, cmp, qd, list, cap);
  if (cnt < 0) return true;
  uint32_t t[N];
  share_terms<N>(cmp, t);
  bool hit = false;
  for (int j = 0; j < cnt && !hit; j += 4) {
    uint32_t h[4], wd[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) h[u] = j + u < cnt ? share_key_of<N>(t, list[(j + u) * 256]) : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) wd[u] = j + u < cnt ? L.sharef[fs_bloom_word(h[u], L.log2_sharef)] : 0u;
#pragma unroll
    for (int u = 0; u < 4; ++u) hit = hit || (j + u < cnt && fs_bloom_test(wd[u], h[u]));
  }
  return hit;
}

// The pairs' test: false when script window s cannot be within the threshold of the fan window whose
// slots' component signatures and squared norms are sg[] / qd[] (sum ff).  A signature is a few bits
// of a hash of the component id (fs_share_sig; FS_NONE: an out-of-vocabulary token), the script
// window's n of them are one 64-bit word: slots whose signatures differ lie in different components,
// slots whose signatures agree count as agreeing.
template <int N>                  // (N = 0: the window size at run time)
__device__ __forceinline__ bool share_pair_possible(const LshDev& L, uint32_t s, uint64_t ssig, const uint32_t* sg,
                                                    const double* qd, double ff) {
  const int n = N ? N : L.n;
  const int b = fs_share_sig_bits(n);
  double af = 0.0;
  uint32_t dm = 0;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const uint32_t c = sg[k];
    const bool far = c == FS_WILD ? false : c == FS_NONE ? true : c != (uint32_t)((ssig >> (k * b)) & ((1u << b) - 1u));
    af = far ? af + qd[k] : af;
    dm |= far ? 1u << k : 0u;
  }
  if (!(ff > 0.0) || dm == 0u) return true;
  // (A >= phi: the bound is at most tau whatever B is)
  if (af >= L.share_phi * (1.0 + 1e-9) * ff) return false;
  const double A = fmin(af / ff, 1.0);
  double bs = 0.0;
#pragma unroll
  for (int k = 0; k < n; ++k)
    if ((dm >> k) & 1u) bs = bs + L.spos[s + k].q;
  const double ss = L.ss[s];
  if (!(ss > 0.0)) return true;
  const double B = fmin(bs / ss, 1.0);
  return sqrt((1.0 - A) * (1.0 - B)) + L.share_gamma * sqrt(A * B) > L.share_tau;
}

// ---- search kernels ------------------------------------------------------------

// The share rule's gate for every window of a token stream: bit w of gbm = window w may have a
// script window within the threshold.  A thread per window, 256 to a workgroup as k_lsh_scan's
// sub-tiles (which read the bits).  A kernel of its own: inside k_lsh_scan its 63 subsets cost a
// wave slot per SIMD (154 registers against 103).
constexpr int kGateCap = 32;
template <int N>
__global__ __launch_bounds__(256) void k_share_gate(CorpusDev c, LshDev L, uint64_t* __restrict__ gbm, uint32_t n_sub) {
  __shared__ uint32_t s_tok[256 + 16], s_cmp[256 + 16];
  __shared__ double s_qd[256 + 16];
  __shared__ share_mask_t<N> s_keys[kGateCap * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t sub = blockIdx.x; sub < n_sub; sub += gridDim.x) {
    const uint64_t p0 = (uint64_t)sub * 256;
    for (int i = threadIdx.x; i < 256 + N - 1; i += 256) {
      const uint32_t id = c.tok[p0 + i];
      s_tok[i] = id;
      s_cmp[i] = share_comp(L, id);
      s_qd[i] = q_of(L, id);
    }
    __syncthreads();
    bool pass = p0 + threadIdx.x + N <= c.n_tok;
    if (pass) pass = share_gate<N>(L, s_cmp + threadIdx.x, s_qd + threadIdx.x, s_keys + threadIdx.x, kGateCap);
    if (L.diag == 4) pass = false;                 // diagnostics: k_lsh_scan's cost with no window to work on
    const uint64_t b = __ballot(pass);
    if (lane == 0) gbm[(size_t)sub * 4 + wave] = b;
    __syncthreads();
  }
}

// The share rule instead of the key scan: the script windows that hold one of a fan window's keys,
// one by one -- the subset keys as an exact map (smap: buckets of four {key, list}, a full bucket
// spills into the next; slists: a key's script windows behind their number) -- through the pairs'
// test and, what is left, the canonical distance.  A pair within the threshold agrees on a heavy
// set of slots, that set contains one of the fan window's minimal heavy subsets, and the script
// window is in that key's list: every script window within the threshold is met, whatever buckets
// it shares with the fan window.  The windows flagged here are therefore a superset of
// k_lsh_scan's (it flags those with a script window within the threshold in a shared bucket); the
// kernels behind it make a window's neighbour list from its buckets and drop a window whose list
// is empty, as behind the other prefilters.  A window the rule does not constrain, or whose work
// finds no room in the workgroup's lists, is flagged as it is.
// One kernel, a workgroup per sub-tile of 256 windows (k_lsh_scan's, and its bitmap), every stage
// dealt out evenly over the 256 threads -- the work per window is very uneven (most windows end
// at the filter, a few have lists of hundreds of script windows):
//   1  a thread per window: its keys (share_asks), the filter; the keys that are there stay;
//   2  a thread per such key: the map -- (window, list) entries;
//   3  a thread per (window, script window) pair of the entries: the pairs' test, the distance.
// workgroups of k_share_scan per CU: the subsets of a window of up to eight slots are bytes (19 KB of
// LDS: seven, at 72 registers; eight measured slower), above that 16 bits (24 KB: six)
constexpr int share_scan_occupancy(int n) { return n <= 8 ? 7 : 6; }
constexpr int kEnumCap = 20;         // keys per window (six slots have at most 20 minimal heavy subsets)
constexpr int kEnumWork = 512;       // keys that are in the filter, and (window, list) entries, per sub-tile
template <int N>
__global__ __launch_bounds__(256, share_scan_occupancy(N)) void k_share_scan(CorpusDev c, LshDev L, uint64_t* __restrict__ qbm,
                                                    uint32_t* __restrict__ qcnt, uint32_t n_sub) {
  __shared__ uint32_t s_tok[256 + 16], s_cmp[256 + 16], s_sg[256 + 16];
  __shared__ double s_qd[256 + 16], s_ff[256];
  __shared__ __attribute__((aligned(16))) share_mask_t<N> s_keys[kEnumCap * 256];   // stage 1: the subsets asked for; stage 3: the entries' offsets (s_wpref)
  __shared__ uint32_t s_hit[kEnumWork], s_wstart[kEnumWork], s_wmeta[kEnumWork];
  __shared__ uint8_t s_found[256];
  __shared__ uint32_t s_w[4], s_nwork, s_ndist;
  uint32_t* s_wpref = reinterpret_cast<uint32_t*>(s_keys);                   // [kEnumWork + 1]
  static_assert((kEnumWork + 1) * 4 <= kEnumCap * 256 * (int)sizeof(share_mask_t<N>) && kEnumWork == 2 * 256, "the offsets take the subsets' place; two entries per thread");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t sub = blockIdx.x; sub < n_sub; sub += gridDim.x) {
    const uint64_t p0 = (uint64_t)sub * 256;
    for (int i = threadIdx.x; i < 256 + N - 1; i += 256) {
      const uint32_t id = c.tok[p0 + i];
      const uint32_t cm = share_comp(L, id);
      s_tok[i] = id;
      s_cmp[i] = cm;
      s_sg[i] = cm >= FS_WILD ? cm : fs_share_sig(cm, N);
      s_qd[i] = q_of(L, id);
    }
    if (threadIdx.x == 0) { s_nwork = 0; s_ndist = 0; }
    s_found[threadIdx.x] = 0;
    __syncthreads();
    // stage 1
    uint32_t hc = 0;
    bool flag = false;
    if (p0 + threadIdx.x + N <= c.n_tok && L.diag != 4) {
      double ff = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) ff = __dadd_rn(ff, s_qd[threadIdx.x + k]);
      s_ff[threadIdx.x] = ff;
      share_mask_t<N>* list = s_keys + threadIdx.x;
      int cnt = share_asks<N>(L, s_cmp + threadIdx.x, s_qd + threadIdx.x, list, kEnumCap);
      flag = cnt < 0;
      if (L.diag == 10) cnt = 0;                                  // diagnostics: the subsets only
      uint32_t t[N];
      share_terms<N>(s_cmp + threadIdx.x, t);
      for (int j = 0; j < cnt; j += 8) {
        uint32_t m[8], h[8], wd[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { m[u] = j + u < cnt ? list[(j + u) * 256] : 0u; h[u] = share_key_of<N>(t, m[u]); }
#pragma unroll
        for (int u = 0; u < 8; ++u) wd[u] = j + u < cnt ? L.sharef[fs_bloom_word(h[u], L.log2_sharef)] : 0u;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (j + u < cnt && fs_bloom_test(wd[u], h[u])) list[hc++ * 256] = (share_mask_t<N>)m[u];   // (hc <= j + u: behind what is read)
      }
      if (L.diag == 6) hc = 0;                                    // diagnostics: no lists
    }
    {
      uint32_t n_hit;
      const uint32_t base = block_excl_scan(hc, s_w, &n_hit);
      for (uint32_t i = 0; i < hc; ++i) {
        if (base + i < (uint32_t)kEnumWork) s_hit[base + i] = threadIdx.x | (uint32_t)s_keys[i * 256 + threadIdx.x] << 8;
        else flag = true;                                         // (no room: the window goes on as it is)
      }
      if (flag) s_found[threadIdx.x] = 1;
      if (L.share_cnt) {                                          // diagnostics: what passes what (fs_index_share_counts)
        const bool in = p0 + threadIdx.x + N <= c.n_tok;
        const uint64_t b0 = __ballot(in), b1 = __ballot(hc > 0), b2 = __ballot(flag);
        if (lane == 0) {
          atomicAdd(L.share_cnt + 0, (unsigned long long)__popcll(b0));
          atomicAdd(L.share_cnt + 1, (unsigned long long)__popcll(b1));
          atomicAdd(L.share_cnt + 6, (unsigned long long)__popcll(b2));
        }
      }
      __syncthreads();
      // stage 2
      const uint32_t bmask = (1u << L.log2_smap) - 1u;
      n_hit = n_hit < (uint32_t)kEnumWork ? n_hit : (uint32_t)kEnumWork;
      for (uint32_t x = threadIdx.x; x < n_hit; x += 256) {
        const uint32_t t = s_hit[x] & 255u, hm = s_hit[x] >> 8;    // the window and the subset: its key again, from the slots' components
        uint32_t tt[N];
        share_terms<N>(s_cmp + t, tt);
        const uint32_t h = share_key_of<N>(tt, hm);
        uint32_t bkt = fs_wmap_slot(h, L.log2_smap);
        for (int probe = 0;; ++probe) {
          if (probe == 64) { s_found[t] = 1; break; }             // (never seen: the window goes on as it is)
          const uint4* bp = reinterpret_cast<const uint4*>(L.smap + 4 * (size_t)bkt);
          const uint4 a = bp[0], b = bp[1];
          const uint32_t key[4] = {a.x, a.z, b.x, b.z}, val[4] = {a.y, a.w, b.y, b.w};
          for (int e = 0; e < 4; ++e) {
            if (!val[e] || key[e] != h) continue;
            const uint32_t len = L.slists[val[e] - 1].x;           // a list: its length, then its script windows
            const uint32_t at = atomicAdd(&s_nwork, 1u);
            if (at < (uint32_t)kEnumWork && len < (1u << 24)) {
              s_wstart[at] = val[e];
              s_wmeta[at] = t << 24 | len;
            } else {
              s_found[t] = 1;                                      // (no room: the window goes on as it is)
            }
          }
          if (!val[3]) break;                                      // (not full: nothing has spilt past it)
          bkt = (bkt + 1) & bmask;
        }
      }
    }
    __syncthreads();
    // stage 3: the entries' offsets among the sub-tile's pairs, then the pairs, pair j to thread j mod 256
    const uint32_t n_work = s_nwork < (uint32_t)kEnumWork ? s_nwork : (uint32_t)kEnumWork;
    uint32_t mine[2], sum = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t e = threadIdx.x * 2 + u;
      mine[u] = e < n_work ? s_wmeta[e] & 0xFFFFFFu : 0u;
      sum += mine[u];
    }
    uint32_t pairs;
    uint32_t at = block_excl_scan(sum, s_w, &pairs);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint32_t e = threadIdx.x * 2 + u;
      if (e < n_work) s_wpref[e] = at;
      at += mine[u];
    }
    if (threadIdx.x == 0) {
      s_wpref[n_work] = pairs;
      if (L.share_cnt) { atomicAdd(L.share_cnt + 2, (unsigned long long)n_work); atomicAdd(L.share_cnt + 3, (unsigned long long)pairs); }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < pairs && L.diag != 5; j += 256) {                            // (diagnostics 5: no pairs)
      uint32_t lo = 0, hi = n_work;                               // s_wpref[lo] <= j < s_wpref[hi]
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_wpref[mid] <= j) lo = mid; else hi = mid;
      }
      const uint32_t t = s_wmeta[lo] >> 24;
      if (s_found[t]) continue;                                   // the window has its answer already
      // (a list's entry: the script window and its signature word, one 16-byte load)
      const uint4 it = L.slists[s_wstart[lo] + (j - s_wpref[lo])];
      const double pff = s_ff[t];
      if (!share_pair_possible<N>(L, it.x, (uint64_t)it.z << 32 | it.y, s_sg + t, s_qd + t, pff) || L.diag == 7) continue;   // (diagnostics 7: no distances)
      // what is left needs the distance: all of the sub-tile's at once behind the loop (a distance
      // inside it holds the thread's wave for four more levels of loads in every pass)
      const uint32_t at = atomicAdd(&s_ndist, 1u);
      if (at < (uint32_t)kEnumWork) {
        s_hit[at] = t << 24 | it.x;                               // (s_hit is free since stage 2; script windows < 2^24: 2^18 at most)
      } else {
        double d;
        if (window_distance_flat<N>(L, it.x, s_tok + t, s_qd + t, pff, __dsqrt_rn(pff), &d) && d < L.thr) s_found[t] = 1;
      }
    }
    __syncthreads();
    {
      const uint32_t nd = s_ndist < (uint32_t)kEnumWork ? s_ndist : (uint32_t)kEnumWork;
      for (uint32_t x = threadIdx.x; x < nd; x += 256) {
        const uint32_t t = s_hit[x] >> 24, sw = s_hit[x] & 0xFFFFFFu;
        if (s_found[t]) continue;
        const double pff = s_ff[t];
        double d;
        if (window_distance_flat<N>(L, sw, s_tok + t, s_qd + t, pff, __dsqrt_rn(pff), &d) && d < L.thr) s_found[t] = 1;
      }
    }
    __syncthreads();
    // thread (wave j, lane l) reports window 4 l + j, as k_lsh_scan does: wave j's ballot is bitmap
    // word j of the sub-tile
    const uint64_t b = __ballot(s_found[4 * lane + wave] != 0);
    if (lane == 0) {
      qbm[(size_t)sub * 4 + wave] = b;
      s_w[wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      qcnt[sub] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
      if (L.share_cnt) {
        atomicAdd(L.share_cnt + 4, (unsigned long long)s_ndist);
        atomicAdd(L.share_cnt + 5, (unsigned long long)(s_w[0] + s_w[1] + s_w[2] + s_w[3]));
      }
    }
    __syncthreads();
  }
}

// 64-bit words of k_lsh_scan's first LDS array: the ballot words of 256 windows in phase 1; in phase 2
// s_ff, s_flag and behind them (384 words in) the share rule's per-token arrays
__host__ __device__ inline int lsh_scan_bal_words(int NW) { return 256 * NW > 800 ? 256 * NW : 800; }
__host__ __device__ inline int lsh_scan_pref_words(int H) { return 256 * H + 1 > 512 ? 256 * H + 1 : 512; }

__global__ __launch_bounds__(256) void k_lsh_scan(CorpusDev c, LshDev L, const uint64_t* __restrict__ gbm,
                                                  uint64_t* __restrict__ qbm,
                                                  uint32_t* __restrict__ qcnt, uint32_t n_sub) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  const int NW = (L.C + 63) >> 6;                    // ballot words per window
  // (LDS is what bounds this kernel's occupancy: 40 KB per workgroup, four per CU.  The
  // ballot words are dead once the keys are assembled and then hold the phase-2 arrays
  // s_ff and s_flag; s_bound, phase 1 only, lies where phase 2 keeps its pair offsets.)
  uint64_t* s_bal = reinterpret_cast<uint64_t*>(s_raw);                 // [256][NW]
  const int bal_words = lsh_scan_bal_words(NW);                         // (room for s_ff + s_flag + the share rule's arrays)
  uint32_t* s_key = reinterpret_cast<uint32_t*>(s_bal + bal_words);     // [256][H]
  uint32_t* s_tok = s_key + 256 * L.H;                                  // [256 + 16]
  uint32_t* s_pref = s_tok + 256 + 16;                                  // [256 * H + 1] pair offsets
  double* s_ff = reinterpret_cast<double*>(s_bal);                      // [256]  (phase 2)
  uint32_t* s_flag = reinterpret_cast<uint32_t*>(s_bal + 256);          // [256]  (phase 2)
  float* s_bound = reinterpret_cast<float*>(s_pref);                    // [256]  (phase 1)
  uint32_t* s_list = s_pref + 256;                                      // [256]  the windows phase 1 makes keys for
  // the share rule's test of the pairs: component id and squared norm per token of the sub-tile
  uint32_t* s_cmp2 = reinterpret_cast<uint32_t*>(s_bal + 384);          // [256 + 16]  (phase 2)
  double* s_qd2 = reinterpret_cast<double*>(s_cmp2 + 272);              // [256 + 16]  (phase 2)
  const bool pair_test = (L.share_flags & 2) != 0;
  __shared__ uint32_t s_cnt[4];
  __shared__ uint64_t s_gate[4];
  __shared__ uint32_t s_nlist;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int n = L.n;
  for (uint32_t sub = blockIdx.x; sub < n_sub; sub += gridDim.x) {
    const uint64_t p0 = (uint64_t)sub * 256;
    for (int i = threadIdx.x; i < 256 + n - 1; i += 256) s_tok[i] = c.tok[p0 + i];
    __syncthreads();
    {
      // the windows that need keys at all: those inside the token stream -- and, under the share
      // rule, through its gate
      bool pass = p0 + threadIdx.x + n <= c.n_tok;
      if (gbm) pass = pass && ((gbm[(size_t)sub * 4 + wave] >> lane) & 1ull);
      const uint64_t b = __ballot(pass);
      if (lane == 0) s_gate[wave] = b;
      __syncthreads();
      uint32_t before = 0;
      for (int j = 0; j < wave; ++j) before += __popcll(s_gate[j]);
      if (pass) s_list[before + __popcll(b & ((1ull << lane) - 1ull))] = threadIdx.x;
      if (threadIdx.x == 255) s_nlist = before + __popcll(b);
    }
    __syncthreads();
    const int n_list = __builtin_amdgcn_readfirstlane((int)s_nlist);
    if ((int)threadIdx.x < n_list) {
      // per window: the float32 decision bound, or -1 when the window needs float64
      const int w = (int)s_list[threadIdx.x];
      float m = 0.0f;
      int terms = 0;
      const bool f64 = L.atab32 == nullptr || (L.diag & 64);       // (diag 64: float64 for OOV windows as before round 5)
      bool oov = false;
      for (int k = 0; k < n; ++k) {
        const uint32_t id = s_tok[w + k];
        oov = oov || (id & FS_OOV_FLAG);
        if (!f64 || !(id & FS_OOV_FLAG)) row32_bound(L, k, id, &m, &terms);
      }
      // (an out-of-vocabulary slot is up to three float32 addends instead of one: the bound's
      // n becomes the number of addends)
      s_bound[w] = (L.atab32 == nullptr || (f64 && oov)) ? -1.0f : key_bound32(L, m, terms);
      s_key[w] = oov ? 1u : 0u;                    // (phase 1 only: s_key is written behind it)
    }
    __syncthreads();
    // phase 1: a wave takes four windows at a time; lane l holds projection columns
    // 4l .. 4l+3 of each, so one 16-byte load per lane fetches a whole table row
    // (848 B at the default 210 columns) per wave instruction.  Only the sign of a
    // projection matters, so the float32 copy of the tables decides it whenever the
    // float32 sum is farther from zero than its worst-case distance to the canonical
    // float64 sum:  |s32 - s64| <= n * 2^-23 * sum_k max_c|A[k][t_k][c]|  (rounding
    // of the n table entries to float32 plus n-1 float32 additions; the float64
    // additions contribute 2^-53 terms; below 2^-126 a rounding is absolute, not
    // relative: key_bound32's second term).  A window with any column inside twice
    // that distance, or with an out-of-vocabulary token, is redone in float64.
    uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_bal);           // [256][2 NW]
    for (int c0 = 0; c0 < L.C && L.diag != 2; c0 += 256) {
      const int col = c0 + 4 * lane;
      const int left = L.C - col;                                    // columns this lane owns
      const uint32_t cmask = left >= 4 ? 0xFu : left > 0 ? (1u << left) - 1 : 0u;
      const int colc = left > 0 ? col : 0;
      const bool store = (lane & 7) == 0 && (c0 >> 5) + (lane >> 3) < 2 * NW;
      for (int g = wave; 4 * g < n_list; g += 4) {
        // (four windows of the list at a time; the last group repeats the list's last window)
        int wl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
          wl[u] = __builtin_amdgcn_readfirstlane((int)s_list[4 * g + u < n_list ? 4 * g + u : n_list - 1]);
        float bnd[4];
        bool fast = true;
#pragma unroll
        for (int u = 0; u < 4; ++u) { bnd[u] = s_bound[wl[u]]; fast = fast && bnd[u] >= 0.0f; }
        uint32_t nib[4];
        bool redo[4] = {true, true, true, true};
        if (fast) {                                                  // wave-uniform
          float4 acc[4];
          // (table rows only -- the common case -- with no branch between the loads; a group
          // of four windows that holds an out-of-vocabulary token takes the rows through row32)
          const bool plain = !(s_key[wl[0]] | s_key[wl[1]] | s_key[wl[2]] | s_key[wl[3]]);
          if (plain) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              acc[u] = *reinterpret_cast<const float4*>(L.atab32 + (size_t)s_tok[wl[u]] * L.Cp + colc);
            for (int k = 1; k < n; ++k) {
              float4 r[4];
#pragma unroll
              for (int u = 0; u < 4; ++u)
                r[u] = *reinterpret_cast<const float4*>(
                    L.atab32 + ((size_t)k * L.V + s_tok[wl[u] + k]) * L.Cp + colc);
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                acc[u].x = __fadd_rn(acc[u].x, r[u].x); acc[u].y = __fadd_rn(acc[u].y, r[u].y);
                acc[u].z = __fadd_rn(acc[u].z, r[u].z); acc[u].w = __fadd_rn(acc[u].w, r[u].w);
              }
            }
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              acc[u] = row32(L, 0, s_tok[wl[u]], colc);
            for (int k = 1; k < n; ++k) {
              float4 r[4];
#pragma unroll
              for (int u = 0; u < 4; ++u)
                r[u] = row32(L, k, s_tok[wl[u] + k], colc);
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                acc[u].x = __fadd_rn(acc[u].x, r[u].x); acc[u].y = __fadd_rn(acc[u].y, r[u].y);
                acc[u].z = __fadd_rn(acc[u].z, r[u].z); acc[u].w = __fadd_rn(acc[u].w, r[u].w);
              }
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const uint32_t sure = (fabsf(acc[u].x) > bnd[u] ? 1u : 0u) | (fabsf(acc[u].y) > bnd[u] ? 2u : 0u) |
                                  (fabsf(acc[u].z) > bnd[u] ? 4u : 0u) | (fabsf(acc[u].w) > bnd[u] ? 8u : 0u);
            nib[u] = ((acc[u].x > 0.0f ? 1u : 0u) | (acc[u].y > 0.0f ? 2u : 0u) |
                      (acc[u].z > 0.0f ? 4u : 0u) | (acc[u].w > 0.0f ? 8u : 0u)) & cmask;
            redo[u] = __any((~sure & cmask) != 0u);                  // wave-uniform
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (redo[u]) {
            uint32_t bits = 0;
            for (int j = 0; j < 4; ++j) {
              if (!((cmask >> j) & 1u)) continue;
              double acc = a_value(L, 0, s_tok[wl[u]], col + j);
              for (int k = 1; k < n; ++k)
                acc = __dadd_rn(acc, a_value(L, k, s_tok[wl[u] + k], col + j));
              bits |= acc > 0.0 ? 1u << j : 0u;
            }
            nib[u] = bits;
          }
          // eight lanes -> one 32-bit piece of the window's column bit string
          uint32_t x = nib[u];
          x |= (uint32_t)__shfl_down((int)x, 1) << 4;
          x |= (uint32_t)__shfl_down((int)x, 2) << 8;
          x |= (uint32_t)__shfl_down((int)x, 4) << 16;
          if (store) s_bits[(size_t)wl[u] * 2 * NW + (c0 >> 5) + (lane >> 3)] = x;
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_list * L.H; i += 256) {
      const int li = i / L.H, h = i - li * L.H, w = (int)s_list[li];
      s_key[w * L.H + h] = assemble_key(s_bal + w * NW, h, L.B);
    }
    __syncthreads();
    // phase 2: "is any bucket candidate of the window within the threshold?"  The 256 x H
    // buckets of the sub-tile hold very different numbers of candidates, so they are not
    // walked window by window: thread w looks up its window's H bucket ranges, a block
    // scan turns the sizes into offsets, and the (window, candidate) pairs of the whole
    // sub-tile are then dealt out evenly, pair j to thread j mod 256 (the bucket of a
    // pair is found by binary search over the offsets in LDS).  A pair that is within
    // the threshold sets its window's flag.
    {
      const int w = threadIdx.x;
      const bool valid = ((s_gate[w >> 6] >> (w & 63)) & 1ull) && L.diag != 1;
      if (pair_test)
        for (int i = threadIdx.x; i < 256 + n - 1; i += 256) {
          const uint32_t id = s_tok[i];
          const uint32_t cm = share_comp(L, id);
          s_cmp2[i] = cm >= FS_WILD ? cm : fs_share_sig(cm, n);
          s_qd2[i] = q_of(L, id);
        }
      const uint32_t nb1 = (1u << L.B) + 1;
      uint32_t sum = 0;
      for (int h = 0; h < L.H; ++h) {
        uint32_t e0 = 0, cntb = 0;
        if (valid) {
          const uint32_t* o = L.boff + (size_t)h * nb1 + s_key[w * L.H + h];
          e0 = o[0];
          cntb = o[1] - e0;
        }
        s_key[w * L.H + h] = e0;                 // the key is not needed again
        s_pref[w * L.H + h] = sum;               // offset inside the window, for now
        sum += cntb;
      }
      double ff = 0.0;
      for (int k = 0; k < n; ++k) ff = __dadd_rn(ff, q_of(L, s_tok[w + k]));
      s_ff[w] = ff;
      s_flag[w] = 0;
      uint32_t total;
      const uint32_t base = block_excl_scan(sum, s_cnt, &total);
      for (int h = 0; h < L.H; ++h) s_pref[w * L.H + h] += base;
      if (w == 255) s_pref[256 * L.H] = total;
      __syncthreads();
      const uint32_t n_b = 256u * (uint32_t)L.H;
      // (round 5 measured this loop two and four pairs at a time, level by level -- bucket entry,
      // the window's record, the first slot's pair-table entry, window_distance's first early exit
      // on those: 2.58 and 3.96 ms per search against 2.41 on the realistic table, where the loop
      // is 58 % of the search.  It is not the latency of one thread's chain that bounds it but
      // the number of random sectors: 134 M pairs per 2 M windows, each with a pair-table entry
      // out of a table far larger than the caches.  The window's record is not one of them: with
      // the records carried in the bucket entries (32 B, in bucket order) the kernel took 5.87 ms
      // against 5.86 ms on 4 M windows.  By switches (FS_LSH_DIAG 1, 3) on those 4 M windows:
      // keys 1.4 ms, the walk without distances 0.7 ms, the distances 2.5 ms)
      for (uint32_t j = threadIdx.x; j < total; j += 256) {
        uint32_t lo = 0, hi = n_b;               // s_pref[lo] <= j < s_pref[hi]
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_pref[mid] <= j) lo = mid; else hi = mid;
        }
        const uint32_t pw = lo / (uint32_t)L.H, ph = lo - pw * (uint32_t)L.H;
        if (s_flag[pw]) continue;                // the window has its answer already
        const uint32_t sidx = L.bids[(size_t)ph * L.W + s_key[lo] + (j - s_pref[lo])];
        if (L.diag == 3) continue;               // diagnostics: bucket walk only
        const double pff = s_ff[pw];
        if (pair_test && !share_pair_possible<0>(L, sidx, L.ssig[sidx], s_cmp2 + pw, s_qd2 + pw, pff)) continue;
        double d;
        if (window_distance(L, sidx, s_tok + pw, nullptr, pff, __dsqrt_rn(pff), &d) && d < L.thr) s_flag[pw] = 1;
      }
      __syncthreads();
    }
    // thread (wave j, lane l) reports window 4 l + j, so that wave j's ballot is bitmap
    // word j of the sub-tile
    const bool flag = s_flag[4 * lane + wave] != 0;
    const uint64_t b = __ballot(flag);
    if (lane == 0) {
      qbm[(size_t)sub * 4 + wave] = b;
      s_cnt[wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) qcnt[sub] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
  }
}

}  // namespace

int fs_launch_lsh_scan(fs_index* ix, const CorpusDev& c, uint64_t* qbm, uint32_t* qcnt,
                       uint32_t n_sub, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (!n_sub) return FS_OK;
  const LshDev L = lsh_dev(ix);
  const int NW = (L.C + 63) >> 6;
  const size_t lds = (size_t)lsh_scan_bal_words(NW) * 8 + (size_t)256 * L.H * 4 + (256 + 16) * 4 +
                     ((size_t)lsh_scan_pref_words(L.H) + 1) * 4;
  FS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lsh_scan),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / (lds + 64)));
  const uint32_t blocks = std::min<uint32_t>(n_sub, ix->num_cu * per_cu);
  const uint64_t* gbm = nullptr;
  if ((L.share_flags & 32) && L.n >= 2 && L.n <= 12) {
    // the share rule by itself: the script windows behind every window's keys
    const uint32_t sblocks = std::min<uint32_t>(n_sub, ix->num_cu * (uint32_t)share_scan_occupancy(L.n));
    switch (L.n) {
#define FS_SHARE_CASE(NN) \
      case NN: hipExtLaunchKernelGGL(k_share_scan<NN>, dim3(sblocks), dim3(256), 0, s, e0, e1, 0u, c, L, qbm, qcnt, n_sub); break;
      FS_SHARE_CASE(2) FS_SHARE_CASE(3) FS_SHARE_CASE(4) FS_SHARE_CASE(5) FS_SHARE_CASE(6) FS_SHARE_CASE(7)
      FS_SHARE_CASE(8) FS_SHARE_CASE(9) FS_SHARE_CASE(10) FS_SHARE_CASE(11) FS_SHARE_CASE(12)
#undef FS_SHARE_CASE
      default: break;
    }
    FS_HIP(hipGetLastError());
    return FS_OK;
  }
  if ((L.share_flags & 1) && L.n >= 2 && L.n <= 12) {
    // the share rule's gate first: the windows that need keys at all
    FS_TRY(ix->cur->w_gate.reserve((size_t)n_sub * 4));
    const uint32_t gblocks = std::min<uint32_t>(n_sub, ix->num_cu * 4);
    uint64_t* g = ix->cur->w_gate.p;
    switch (L.n) {
#define FS_SHARE_CASE(NN) \
      case NN: hipExtLaunchKernelGGL(k_share_gate<NN>, dim3(gblocks), dim3(256), 0, s, e0, nullptr, 0u, c, L, g, n_sub); break;
      FS_SHARE_CASE(2) FS_SHARE_CASE(3) FS_SHARE_CASE(4) FS_SHARE_CASE(5) FS_SHARE_CASE(6) FS_SHARE_CASE(7)
      FS_SHARE_CASE(8) FS_SHARE_CASE(9) FS_SHARE_CASE(10) FS_SHARE_CASE(11) FS_SHARE_CASE(12)
#undef FS_SHARE_CASE
      default: break;
    }
    FS_HIP(hipGetLastError());
    if (ix->prof.on) fs_prof_mark(ix, s, "k_share_gate");
    e0 = nullptr;
    gbm = g;
  }
  hipExtLaunchKernelGGL(k_lsh_scan, dim3(blocks), dim3(256), (uint32_t)lds, s, e0, e1, 0u, c, L, gbm, qbm,
                        qcnt, n_sub);
  FS_HIP(hipGetLastError());
  return FS_OK;
}
