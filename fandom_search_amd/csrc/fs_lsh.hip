// fs_lsh.hip -- the general pipeline: the reference's algorithm as written.  Its units: fs_lsh.h.
//
// Every fan window is hashed with all H random-binary-projection tables, every
// bucket candidate is scored with the cosine distance, NearestFilter keeps the N
// nearest, the threshold keeps those below `distance_threshold`
// (`search.py` of the reference, 112-123 and 176-184, and NearPy's Engine).
// Used whenever the exact n-gram proof does not hold: window sizes for which one
// substituted token can stay within the threshold (n = 8, 10 on the synthetic
// table), out-of-vocabulary tokens, vector tables with near-duplicate rows.
//
//   RandomBinaryProjections.hash_vector   window_keys: per-token projection
//        tables A[k][v][c] (k_atab), window projection = sum over k in order,
//        key bit = (p > 0.0); canonical arithmetic of DESIGN.md section 3
//   Engine.store_vector                   fs_lsh_build (fs_lsh_build.hip): script window keys
//        and CSR buckets per table (ascending window index) on the device
//   Engine.neighbours                     lsh_neighbours: bucket entries of
//        table 0, 1, ... in order, UniqueFilter by script window, cosine
//        distance (canonical), stable NearestFilter(N), threshold
//
// The kernels of this file, for the windows the sift leaves pending:
//   k_lsh_verify   one wave per pending window (lsh_window): keys again, the full
//                  neighbours list, Levenshtein per kept match, best rank ->
//                  per-candidate record for k_rows
//   k_lsh_gramtab  lsh_window once per script n-gram and string table
//   k_lsh_batch    eight pending windows per wave, the same steps level by level
//   k_lsh_pkeys, k_lsh_enum    in front of k_lsh_batch where the script n-grams one slot away
//                  can be enumerated: the windows' keys, then their neighbour lists without a
//                  bucket walk; k_lsh_batch takes what they leave
//   k_lsh_lev      the kept matches' Levenshtein distances a lane per match, and the records,
//                  behind k_lsh_verify<true> / k_lsh_batch / k_lsh_enum
// fs_launch_lsh_verify fills LshDev for a search, launches the sift (fs_lsh_sift.hip) and then
// the kernels above (lsh_launch_pending).
//
// A candidate's exact distance is skipped only when a sound upper bound on its
// cosine is already below 1 - threshold: too few identical slots for the table's
// c_max (integer test), or, slot by slot, the partial canonical sum plus the
// Cauchy-Schwarz bound of the remaining slots (window_distance).  Skipped
// candidates can never be in the output, so the result equals the oracle's, which
// computes every distance.
#include "fs_lsh.h"

#include <hip/hip_ext.h>

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

using namespace fsdev;

namespace {

// Engine.neighbours + threshold.  ANY: stop at the first candidate within the
// threshold (return 1).  Otherwise fill top_s/top_d (capacity nn) with the kept
// matches in NearestFilter order and return their number.
template <bool ANY>
__device__ int lsh_neighbours(const LshDev& L, const uint32_t* keys, const uint32_t* f,
                              uint32_t* top_s, double* top_d) {
  double ff = 0.0;
  for (int k = 0; k < L.n; ++k) ff = __dadd_rn(ff, q_of(L, f[k]));
  const double rff = __dsqrt_rn(ff);
  const uint32_t nb1 = (1u << L.B) + 1;
  int cnt = 0;
  for (int h = 0; h < L.H; ++h) {
    const uint32_t* o = L.boff + (size_t)h * nb1 + keys[h];
    const uint32_t e0 = o[0], e1 = o[1];
    for (uint32_t e = e0; e < e1; ++e) {
      const uint32_t s = L.bids[(size_t)h * L.W + e];
      if (!ANY && L.unique) {
        bool seen = false;
        for (int t = 0; t < cnt; ++t) seen = seen || top_s[t] == s;
        if (seen) continue;
      }
      double d;
      if (L.diag == 3) { cnt += s == 0xFFFFFFFFu; continue; }          // diagnostics: bucket walk only
      if (!window_distance(L, s, f, nullptr, ff, rff, &d)) continue;
      if (!(d < L.thr)) continue;
      if (ANY) return 1;
      // stable insertion: behind every entry with distance <= d
      int pos = cnt;
      while (pos > 0 && d < top_d[pos - 1]) --pos;
      if (pos >= L.nn) continue;
      const int last = cnt < L.nn ? cnt : L.nn - 1;
      for (int m = last; m > pos; --m) { top_d[m] = top_d[m - 1]; top_s[m] = top_s[m - 1]; }
      top_d[pos] = d; top_s[pos] = s;
      if (cnt < L.nn) ++cnt;
    }
  }
  return cnt;
}

// The same neighbour list computed by a whole wave (all 64 lanes call it with the same
// arguments; `keys`, `f`, `top_s`, `top_d`, `s_pre`, `s_e0` in LDS, private to the wave).
// Lane h reads the bucket range of table h; the bucket entries of table 0, 1, ... are
// numbered in order and dealt to the lanes, 64 - nn at a time, behind the <= nn entries
// kept so far: every lane fetches its script window and computes its distance (the
// dependent loads of all candidates in flight together), UniqueFilter = not equal to a
// kept entry or to an earlier lane of the round (an entry dropped earlier has the same
// distance and would be dropped again), NearestFilter = rank in the stable order
// (distance, then arrival) below nn.  Equal to lsh_neighbours<false> entry for entry.
__device__ int lsh_neighbours_wave(const LshDev& L, const uint32_t* keys, const uint32_t* f,
                                   uint32_t* top_s, double* top_d, uint32_t* s_pre,
                                   uint32_t* s_e0, double* qf) {
  const int lane = threadIdx.x & 63;
  if (lane < L.n) qf[lane] = q_of(L, f[lane]);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double ff = 0.0;
  for (int k = 0; k < L.n; ++k) ff = __dadd_rn(ff, qf[k]);
  const double rff = __dsqrt_rn(ff);
  const uint32_t nb1 = (1u << L.B) + 1;
  uint32_t e0 = 0, cnt_h = 0;
  if (lane < L.H) {
    const uint32_t* o = L.boff + (size_t)lane * nb1 + keys[lane];
    e0 = o[0];
    cnt_h = o[1] - e0;
  }
  const uint32_t incl = wave_incl_scan_dpp(cnt_h);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
  s_pre[lane] = incl - cnt_h;                  // lanes >= H: = total
  s_e0[lane] = e0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t nn = (uint32_t)L.nn;
  const uint32_t R = 64 - nn;                  // new candidates per round
  uint32_t kcnt = 0;
  for (uint32_t r0 = 0; r0 < total; r0 += R) {
    const uint32_t m = total - r0 < R ? total - r0 : R;
    uint32_t s = FS_NONE;
    double d = 0.0;
    bool valid = false;
    if ((uint32_t)lane < kcnt) {               // kept so far, in rank order
      s = top_s[lane]; d = top_d[lane]; valid = true;
    } else if ((uint32_t)lane - kcnt < m) {
      const uint32_t j = r0 + ((uint32_t)lane - kcnt);
      uint32_t h = 0;                          // last table with s_pre[h] <= j
#pragma unroll
      for (uint32_t step = 32; step > 0; step >>= 1)
        if (h + step < (uint32_t)L.H && s_pre[h + step] <= j) h += step;
      s = L.bids[(size_t)h * L.W + s_e0[h] + (j - s_pre[h])];
      if (L.diag != 3) valid = window_distance(L, s, f, qf, ff, rff, &d) && d < L.thr;
    }
    if (L.unique) {
      // not the window of a kept entry or of an earlier lane of this round.  Only lanes within
      // the threshold are looked at: a second entry of a window that is not has the same
      // distance and is dropped like the first (two or three lanes instead of every bucket
      // entry: the loop is scalar work, which this kernel is short of)
      uint64_t live = __ballot(valid);
      bool dup = false;
      while (live) {
        const int l = __ffsll((unsigned long long)live) - 1;
        live &= live - 1;
        const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)s, l);
        dup = dup || (l < lane && sl == s);
      }
      if ((uint32_t)lane >= kcnt) valid = valid && !dup;
    }
    // rank in the stable order: smaller distance first, earlier arrival first
    uint64_t vm = __ballot(valid);
    const uint32_t nvalid = (uint32_t)__popcll(vm);
    uint32_t rank = 0;
    const uint32_t dlo = (uint32_t)__double_as_longlong(d), dhi = (uint32_t)(__double_as_longlong(d) >> 32);
    while (vm) {
      const int l = __ffsll((unsigned long long)vm) - 1;
      vm &= vm - 1;
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)dlo, l);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)dhi, l);
      const double dl = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
      rank += (dl < d || (dl == d && l < lane)) ? 1u : 0u;
    }
    __builtin_amdgcn_wave_barrier();           // every lane has read its kept entry
    if (valid && rank < nn) { top_s[rank] = s; top_d[rank] = d; }
    kcnt = nvalid < nn ? nvalid : nn;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  return (int)kcnt;
}

// The LDS a wave needs for one window (private to the wave).
struct LshWaveLds {
  uint64_t* bal;      // [32] sign ballots of the projection columns
  uint32_t* key;      // [64]
  uint32_t* top_s;    // [64] kept matches in NearestFilter order
  double* top_d;      // [64]
  uint32_t* lev;      // [64]
  uint32_t *la, *lb;  // [FS_LEV_MAX + 2] Levenshtein operands
  uint32_t* f;        // [FS_MAX_WINDOW] vector ids of the window
  uint32_t* fs;       // [FS_MAX_WINDOW] string ids of the window
  int* n;             // [1]
  uint32_t *pre, *e0; // [64]
  double* qf;         // [FS_MAX_WINDOW] q of the window's slots
};

// What the reference returns for one fan window, worked out by a whole wave (all 64 lanes
// call it with the same arguments): keys of the window (search.py:176 -> nearpy), the
// buckets' members with their canonical distances, threshold, NearestFilter, the
// Levenshtein distance of every kept match (search.py:189-190) and the first minimum of
// dist * lev in rank order.  S.f / S.fs hold the window's vector and string ids.  Returns the
// number of kept matches; *b (lane 0) is the record when that is not 0.
// `defer`: stop behind the neighbour list (S.top_s / S.top_d hold it): the Levenshtein distances and
// the first minimum are then k_lsh_lev's, a lane per kept match.
__device__ __forceinline__ int lsh_window(const CorpusDev& c, const LshDev& L, const GramIndexDev& g,
                                          const LshWaveLds& S, fs_status* st, fs_best* b, bool defer = false) {
  const int lane = threadIdx.x & 63;
  const int NW = (L.C + 63) >> 6;
  // keys.  Fast path as in k_lsh_scan: lane l holds projection columns 4l .. 4l+3, one
  // 16-byte load per lane and slot fetches the float32 row, all slots requested together;
  // the float32 sums decide the signs when every column is farther from zero than the
  // worst-case distance to the canonical float64 sum, else (and with an OOV token) the
  // window is redone in float64.
  bool keys_done = false;
  if (L.atab32 && L.C <= 256 && !(L.diag & 8)) {
    float am = 0.0f;
    int terms = 0;
    bool oov = false;
    if (lane < L.n) {
      const uint32_t id = S.f[lane];
      oov = (id & FS_OOV_FLAG) != 0 && (L.diag & 64);              // (diag 64: float64 for OOV windows as before round 5)
      if (!oov) row32_bound(L, lane, id, &am, &terms);
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) { am += __shfl_xor(am, d); terms += __shfl_xor(terms, d); }   // n <= 16 lanes hold a value
    am = __shfl(am, 0);
    terms = __shfl(terms, 0);
    if (!__any(oov)) {
      const float bnd = key_bound32(L, am, terms);
      const int col = 4 * lane;
      const int left = L.C - col;
      const uint32_t cmask = left >= 4 ? 0xFu : left > 0 ? (1u << left) - 1 : 0u;
      const int colc = left > 0 ? col : 0;
      // (eight rows in flight at a time; summed in slot order like k_lsh_scan)
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      for (int k0 = 0; k0 < L.n; k0 += 8) {
        float4 r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k0 + k < L.n)
            r[k] = row32(L, k0 + k, S.f[k0 + k], colc);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (k0 + k < L.n) {
            if (k0 + k == 0) { acc = r[0]; continue; }
            acc.x = __fadd_rn(acc.x, r[k].x); acc.y = __fadd_rn(acc.y, r[k].y);
            acc.z = __fadd_rn(acc.z, r[k].z); acc.w = __fadd_rn(acc.w, r[k].w);
          }
      }
      const uint32_t sure = (fabsf(acc.x) > bnd ? 1u : 0u) | (fabsf(acc.y) > bnd ? 2u : 0u) |
                            (fabsf(acc.z) > bnd ? 4u : 0u) | (fabsf(acc.w) > bnd ? 8u : 0u);
      if (!__any((~sure & cmask) != 0u)) {
        uint32_t x = ((acc.x > 0.0f ? 1u : 0u) | (acc.y > 0.0f ? 2u : 0u) |
                      (acc.z > 0.0f ? 4u : 0u) | (acc.w > 0.0f ? 8u : 0u)) & cmask;
        // eight lanes -> one 32-bit piece of the column bit string
        x |= (uint32_t)__shfl_down((int)x, 1) << 4;
        x |= (uint32_t)__shfl_down((int)x, 2) << 8;
        x |= (uint32_t)__shfl_down((int)x, 4) << 16;
        uint32_t* pieces = reinterpret_cast<uint32_t*>(S.bal);
        if ((lane & 7) == 0 && (lane >> 3) < 2 * NW) pieces[lane >> 3] = x;
        keys_done = true;
      }
    }
  }
  for (int ch = 0; ch < NW && !keys_done; ++ch) {
    const int col = ch * 64 + lane;
    bool bit = false;
    if (col < L.C && !(L.diag & 8)) {
      double acc = a_value(L, 0, S.f[0], col);
      for (int k = 1; k < L.n; ++k) acc = __dadd_rn(acc, a_value(L, k, S.f[k], col));
      bit = acc > 0.0;
    }
    const uint64_t b = __ballot(bit);
    if (lane == 0) S.bal[ch] = b;
  }
  if (lane == 0) S.bal[NW] = 0;
  __builtin_amdgcn_wave_barrier();
  if (lane < L.H) S.key[lane] = assemble_key(S.bal, lane, L.B);
  __builtin_amdgcn_wave_barrier();
  int cnt;
  if (L.diag & 32) {
    cnt = 0;
  } else if (L.nn <= 48 && L.H <= 64 && !L.serial_neighbours) {
    cnt = lsh_neighbours_wave(L, S.key, S.f, S.top_s, S.top_d, S.pre, S.e0, S.qf);
  } else {                                    // NearestFilter(N > 48): one lane walks the buckets
    if (lane == 0)
      S.n[0] = lsh_neighbours<false>(L, S.key, S.f, S.top_s, S.top_d);
    __builtin_amdgcn_wave_barrier();
    cnt = S.n[0];
  }
  if (cnt == 0 || defer) return cnt;
  // Levenshtein of every kept match (search.py:189-190), the wave working on one
  // match at a time
  for (int r = 0; r < cnt; ++r) {
    uint32_t lv = FS_NONE;
    if (L.selflev) {
      // a match with the same id in every slot has the same strings as the script window's
      // own ids: its distance was computed once per string table (k_selflev)
      const uint32_t sr = S.top_s[r];
      const bool differs = lane < L.n && L.stok[sr + lane] != S.f[lane];
      if (!__any(differs)) lv = L.selflev[sr];
    }
    if (lv == FS_NONE)
      lv = (L.diag & 16) ? 1u :
                        lev_wave(g, S.top_s[r], S.fs, c.chars, c.coff, c.n_str, st,
                                 S.la, S.lb);
    if (lane == 0) S.lev[r] = lv;
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    b->pad = 0.0;
    for (int r = 0; r < cnt; ++r) {           // first minimum of dist * lev in rank order
      const double comb = __dmul_rn(S.top_d[r], (double)S.lev[r]);
      if (r == 0 || comb < b->comb) {
        b->s = S.top_s[r]; b->lev = S.lev[r]; b->dist = S.top_d[r]; b->comb = comb;
      }
    }
  }
  return cnt;
}

#define FS_LSH_WAVE_LDS                                                                       \
  __shared__ uint64_t s_bal[4][32];                                                           \
  __shared__ uint32_t s_key[4][64];                                                           \
  __shared__ uint32_t s_top_s[4][64];                                                         \
  __shared__ double s_top_d[4][64];                                                           \
  __shared__ uint32_t s_lev[4][64];                                                           \
  __shared__ uint32_t s_la[4][FS_LEV_MAX + 2], s_lb[4][FS_LEV_MAX + 2];                       \
  __shared__ uint32_t s_f[4][FS_MAX_WINDOW];                                                  \
  __shared__ uint32_t s_fs[4][FS_MAX_WINDOW];                                                 \
  __shared__ int s_n[4];                                                                      \
  __shared__ uint32_t s_pre[4][64], s_e0[4][64];                                              \
  __shared__ double s_qf[4][FS_MAX_WINDOW];                                                   \
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));                   \
  const LshWaveLds S{s_bal[wave], s_key[wave], s_top_s[wave], s_top_d[wave], s_lev[wave],     \
                     s_la[wave], s_lb[wave], s_f[wave], s_fs[wave], &s_n[wave], s_pre[wave],   \
                     s_e0[wave], s_qf[wave]}

// Per script n-gram, once per string table (fs_corpus_update_end, like the exact path's
// ctab): what a fan window with the n-gram's ids and the strings of those ids gets.  The
// reference's result for a window is a function of its vector (i.e. of its ids) and, for the
// Levenshtein distances, of its strings, so every such window of a batch takes this record
// (k_lsh_sift) and no bucket is walked for it.  tab_cnt = kept matches + 1.  One wave per
// n-gram.
__global__ __launch_bounds__(256, 4) void k_lsh_gramtab(CorpusDev c, LshDev L, GramIndexDev g,
                                                        unsigned long long* __restrict__ tab_best,
                                                        uint32_t* __restrict__ tab_cnt, fs_status* st) {
  FS_LSH_WAVE_LDS;
  const int lane = threadIdx.x & 63;
  for (uint32_t gram = blockIdx.x * 4 + wave; gram < g.n_grams; gram += gridDim.x * 4) {
    const uint32_t first = g.gpos[(size_t)gram * g.nn];
    if (lane < L.n) {
      const uint32_t id = g.stok[first + lane];
      S.f[lane] = id;
      S.fs[lane] = id;
    }
    __builtin_amdgcn_wave_barrier();
    fs_best b;
    const int cnt = lsh_window(c, L, g, S, st, &b);
    if (lane == 0) {
      if (cnt) {
        const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&b);
#pragma unroll
        for (int k = 0; k < 4; ++k) tab_best[4 * (size_t)gram + k] = src[k];
      }
      tab_cnt[gram] = (uint32_t)cnt + 1u;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// (five waves per SIMD: 94 registers with two spilt; 97 at four.  A wave per window and about ten
// levels of dependent loads: the windows in flight are what counts -- n = 10: 0.268 -> 0.249 ms per
// C2 batch; six waves, 80 registers, eight spilt, measured slower again)
template <bool DEFER>
__global__ __launch_bounds__(256, 5) void k_lsh_verify(CorpusDev c, LshDev L, GramIndexDev g,
                                                    const uint32_t* __restrict__ cpos, NSrc nc,
                                                    uint32_t* __restrict__ cg,
                                                    uint32_t* __restrict__ cw,
                                                    fs_best* __restrict__ cbest,
                                                    uint32_t* __restrict__ bmatch, fs_status* st,
                                                    const uint32_t* __restrict__ pend,
                                                    uint32_t* __restrict__ mcnt,
                                                    uint32_t* __restrict__ mtop_s,
                                                    double* __restrict__ mtop_d) {
  FS_LSH_WAVE_LDS;
  __shared__ uint32_t s_w32[4];
  const int lane = threadIdx.x & 63;
  uint32_t matches = 0;
  // k_lsh_sift has been over every candidate: what it left pending is worked out here, a wave
  // per window, the windows of its list dealt round-robin over the waves.
  const uint32_t gw = blockIdx.x * 4 + wave, NWAVES = gridDim.x * 4;
  const uint32_t n_pend = min(st->lsh_pending, nc.cap);
  {
    for (uint32_t j = gw; j < n_pend; j += NWAVES) {
      const uint32_t i = pend[j];
      const uint64_t p = cpos[i];
      bool ok = p + L.n <= c.n_tok;
      uint32_t w = 0;
      if (ok) {
        uint64_t work_end;
        w = work_of_token(c, p, &work_end);
        ok = p + L.n <= work_end;                 // a window never crosses a work boundary
      }
      if (!ok) {                                  // wave-uniform
        if (lane == 0) { cg[i] = FS_NONE; if (DEFER) mcnt[j] = 0; }
        continue;
      }
      if (lane < L.n) {
        S.f[lane] = c.tok[p + lane];
        S.fs[lane] = c.str ? c.str[p + lane] : c.tok[p + lane];
      }
      __builtin_amdgcn_wave_barrier();
      fs_best b;
      const int cnt = lsh_window(c, L, g, S, st, &b, DEFER);
      if (DEFER) {
        // the kept matches in NearestFilter order for k_lsh_lev (a lane per match there)
        if (lane < cnt) {
          mtop_s[(size_t)j * L.nn + lane] = S.top_s[lane];
          mtop_d[(size_t)j * L.nn + lane] = S.top_d[lane];
        }
        if (lane == 0) {
          mcnt[j] = (uint32_t)cnt;
          cg[i] = cnt ? FS_PENDING : FS_NONE;
          cw[i] = w;
          matches += (uint32_t)cnt;
        }
      } else if (lane == 0) {
        if (cnt) {
          cbest[i] = b;
          cg[i] = 0;
          cw[i] = w;
          matches += (uint32_t)cnt;
        } else {
          cg[i] = FS_NONE;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  uint32_t tot;
  block_excl_scan(matches, s_w32, &tot);
  if (threadIdx.x == 0) bmatch[blockIdx.x] += tot;       // (on top of k_lsh_sift's)
}

// ---- the pending windows eight at a time (round 5) ----------------------------------------
// k_lsh_verify works a window off with a whole wave: keys, bucket ranges, bucket members,
// distances, NearestFilter -- about ten levels of dependent loads for one window, during most
// of which most lanes wait (71 % of the wave cycles waiting, r04_lsh_verify_pmc_sq_after.json),
// and on a table with near-synonyms a C2 batch leaves 280 k such windows: 0.85 of the search's
// 1.05 ms.  k_lsh_batch takes EIGHT windows of the pending list per wave and walks the same
// steps level by level for all of them at once:
//   A  ids, q and bounds of the eight windows, lane per (window, slot); float32 projection rows
//      summed in slot order, four columns a lane (float64 redo per window where a sign is not
//      certain, as lsh_window)
//   B  the 8 x H bucket ranges, lane per (window, table)
//   C  the bucket members of all eight windows numbered in (window, table, entry) order and
//      dealt to the lanes 64 at a time: script window, canonical distance (window_distance);
//      those within the threshold go to the window's list in LDS in arrival order
//   D  UniqueFilter and NearestFilter per window, eight lanes a window: an entry's rank in the
//      stable order (distance, then arrival) among the entries that are not repeats
// What it keeps equals lsh_neighbours_wave's list entry for entry (NearPy: UniqueFilter keeps a
// window's first arrival, NearestFilter is a stable sort).  A window with more than kBatchCap
// members within the threshold (crowded buckets) is worked off by lsh_window behind the batch.
// The Levenshtein distances are k_lsh_lev's (a lane per kept match).
constexpr int kBatchW = 8;                // windows per wave and step
constexpr int kBatchCap = 32;             // members within the threshold kept per window
constexpr int kBatchH = 16;               // tables (number_of_hashes) this form serves
constexpr int kBatchBal = (kBatchH * 24 + 63) / 64 + 1;   // words per window: C <= 16 * 24 columns + a zero word
struct alignas(16) BatchLds {             // per wave
  uint64_t bal[kBatchW][kBatchBal];       // sign bits of the projection columns, + a zero word
  double qf[kBatchW][FS_MAX_WINDOW];      // q of the windows' slots
  double ff[kBatchW], rff[kBatchW];
  double vd[kBatchW][kBatchCap];          // members within the threshold, arrival order: distance ...
  uint32_t vs[kBatchW][kBatchCap];        // ... and script window (bit 31: a repeat)
  uint32_t f[kBatchW][FS_MAX_WINDOW];     // vector ids
  uint32_t key[kBatchW][kBatchH];
  uint32_t e0[kBatchW][kBatchH];          // first entry of the window's bucket in table h
  uint32_t pre[kBatchW][kBatchH];         // entries of the window in the tables before h
  uint32_t dh[128];                       // C: (window, script window) -> a lane of the round that holds the pair
  uint32_t jj[kBatchW];                   // the window's place in the pending list (mcnt / mtop)
  uint32_t wbase[kBatchW + 1];            // entries of the windows before w
  uint32_t vn[kBatchW];                   // members within the threshold so far (may exceed kBatchCap)
  uint32_t ci[kBatchW];                   // candidate number
  uint32_t work[kBatchW];
  uint32_t ok[kBatchW];                   // 1: a window of one work; 2: its keys need float64
  float bnd[kBatchW];
};
static_assert(sizeof(double) * kBatchW * kBatchCap + sizeof(uint32_t) * kBatchW * kBatchCap >= 2400,
              "lsh_window's scratch is laid over vd / vs");

template <int N>
__global__ __launch_bounds__(256, 5) void k_lsh_batch(CorpusDev c, LshDev L, GramIndexDev g,
                                                   const uint32_t* __restrict__ cpos, uint32_t cap,
                                                   uint32_t* __restrict__ cg, uint32_t* __restrict__ cw,
                                                   uint32_t* __restrict__ bmatch, fs_status* st,
                                                   const uint32_t* __restrict__ pend,
                                                   uint32_t* __restrict__ mcnt,
                                                   uint32_t* __restrict__ mtop_s,
                                                   double* __restrict__ mtop_d,
                                                   const uint32_t* __restrict__ left,
                                                   const uint32_t* __restrict__ n_left) {
  __shared__ BatchLds s_b[4];
  __shared__ uint32_t s_w32[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  BatchLds& S = s_b[wave];
  uint32_t matches = 0;
  const uint32_t gw = blockIdx.x * 4 + wave, NWAVES = gridDim.x * 4;
  // (left: the windows k_lsh_enum could not finish, as places in the pending list)
  const uint32_t n_pend = left ? min(*n_left, cap) : min(st->lsh_pending, cap);
  const uint32_t nn = (uint32_t)L.nn;
  const uint32_t nb1 = (1u << L.B) + 1;
  auto sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  // (few windows: fewer per wave, so that every wave has some -- a wave's eight windows take
  // a hundred microseconds when each walks sixty bucket members)
  const uint32_t per = max(1u, min((uint32_t)kBatchW, (n_pend + NWAVES - 1) / NWAVES));
  if ((L.diag & 0x100000) && left && blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&st->max_rows, n_pend);   // diagnostics: windows left to the walk
  for (uint32_t j0 = gw * per; j0 < n_pend; j0 += NWAVES * per) {
    const uint32_t nw = min(per, n_pend - j0);
    // ---- A: the windows ------------------------------------------------------------------
    if (lane < kBatchW) {
      uint32_t ok = 0, w = 0, i = 0;
      uint64_t p = 0;
      uint32_t jx = 0;
      if ((uint32_t)lane < nw) {
        jx = left ? left[j0 + lane] : j0 + lane;
        i = pend[jx];
        p = cpos[i];
        if (p + N <= c.n_tok) {
          uint64_t work_end;
          w = work_of_token(c, p, &work_end);
          ok = p + N <= work_end ? 1u : 0u;       // a window never crosses a work boundary
        }
      }
      S.ci[lane] = i; S.work[lane] = w; S.ok[lane] = ok; S.vn[lane] = 0; S.jj[lane] = jx;
      S.wbase[lane] = (uint32_t)p;                // (the position, until B overwrites it)
      S.bal[lane][(L.C + 63) >> 6] = 0;
    }
    sync();
#pragma unroll
    for (int t = 0; t < kBatchW * FS_MAX_WINDOW / 64; ++t) {      // lane per (window, slot)
      const int w = (t * 64 + lane) / FS_MAX_WINDOW, k = (t * 64 + lane) % FS_MAX_WINDOW;
      float am = 0.0f;
      int terms = 0;
      uint32_t oov = 0;
      if (k < N && S.ok[w]) {
        const uint32_t id = c.tok[(uint64_t)S.wbase[w] + k];
        S.f[w][k] = id;
        S.qf[w][k] = q_of(L, id);
        oov = (L.diag & 64) ? id & FS_OOV_FLAG : 0u;                // (diag 64: float64 for OOV windows as before round 5)
        if (!oov && L.atab32) row32_bound(L, k, id, &am, &terms);
      }
      // sum / or over the window's FS_MAX_WINDOW lanes
      static_assert(FS_MAX_WINDOW == 16, "a window's slots are one row of sixteen lanes");
#pragma unroll
      for (int d = 8; d > 0; d >>= 1) { am += __shfl_xor(am, d); terms += __shfl_xor(terms, d); oov |= (uint32_t)__shfl_xor((int)oov, d); }
      if (k == 0 && S.ok[w]) {
        S.bnd[w] = key_bound32(L, am, terms);
        if (oov || !L.atab32 || L.C > 256) S.ok[w] = 2u;
      }
    }
    sync();
    if (lane < kBatchW && S.ok[lane]) {
      double ff = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) ff = __dadd_rn(ff, S.qf[lane][k]);
      S.ff[lane] = ff;
      S.rff[lane] = __dsqrt_rn(ff);
    }
    // keys, float32: lane l holds projection columns 4l .. 4l+3; the N rows of a window
    // requested together, summed in slot order (as lsh_window)
    {
      const int col = 4 * lane;
      const int left = L.C - col;
      const uint32_t cmask = left >= 4 ? 0xFu : left > 0 ? (1u << left) - 1 : 0u;
      const int colc = left > 0 ? col : 0;
      // (the rows of two windows in flight together where the registers allow: n <= 8)
      constexpr int PAIR = N <= 8 ? 2 : 1;
      auto finish = [&](uint32_t w, float4 acc) {
        const float bnd = S.bnd[w];
        const uint32_t sure = (fabsf(acc.x) > bnd ? 1u : 0u) | (fabsf(acc.y) > bnd ? 2u : 0u) |
                              (fabsf(acc.z) > bnd ? 4u : 0u) | (fabsf(acc.w) > bnd ? 8u : 0u);
        if (__any((~sure & cmask) != 0u)) {
          if (lane == 0) S.ok[w] = 2u;            // a sign is not certain: float64 below
          return;
        }
        uint32_t x = ((acc.x > 0.0f ? 1u : 0u) | (acc.y > 0.0f ? 2u : 0u) |
                      (acc.z > 0.0f ? 4u : 0u) | (acc.w > 0.0f ? 8u : 0u)) & cmask;
        // eight lanes -> one 32-bit piece of the column bit string
        x |= (uint32_t)__shfl_down((int)x, 1) << 4;
        x |= (uint32_t)__shfl_down((int)x, 2) << 8;
        x |= (uint32_t)__shfl_down((int)x, 4) << 16;
        uint32_t* pieces = reinterpret_cast<uint32_t*>(S.bal[w]);
        if ((lane & 7) == 0) pieces[lane >> 3] = x;
      };
      for (uint32_t w0 = 0; w0 < nw; w0 += PAIR) {
        float4 r[PAIR][N];
        bool go[PAIR];
#pragma unroll
        for (int u = 0; u < PAIR; ++u) {
          go[u] = w0 + u < nw && S.ok[w0 + u] == 1u;             // (wave-uniform)
          if (go[u]) {
#pragma unroll
            for (int k = 0; k < N; ++k)
              r[u][k] = row32(L, k, S.f[w0 + u][k], colc);
          }
        }
#pragma unroll
        for (int u = 0; u < PAIR; ++u)
          if (go[u]) {
            float4 acc = r[u][0];
#pragma unroll
            for (int k = 1; k < N; ++k) {
              acc.x = __fadd_rn(acc.x, r[u][k].x); acc.y = __fadd_rn(acc.y, r[u][k].y);
              acc.z = __fadd_rn(acc.z, r[u][k].z); acc.w = __fadd_rn(acc.w, r[u][k].w);
            }
            finish(w0 + u, acc);
          }
      }
    }
    sync();
    for (uint32_t w = 0; w < nw; ++w) {           // float64 keys where needed (rare)
      if (S.ok[w] != 2u) continue;
      for (int ch = 0; ch < (L.C + 63) >> 6; ++ch) {
        const int col = ch * 64 + lane;
        bool bit = false;
        if (col < L.C) {
          double acc = a_value(L, 0, S.f[w][0], col);
          for (int k = 1; k < N; ++k) acc = __dadd_rn(acc, a_value(L, k, S.f[w][k], col));
          bit = acc > 0.0;
        }
        const uint64_t b = __ballot(bit);
        if (lane == 0) S.bal[w][ch] = b;
      }
    }
    sync();
    if (L.diag & 0x10000) {                       // diagnostics: the keys only
      if (lane < kBatchW && (uint32_t)lane < nw) { mcnt[S.jj[lane]] = 0; cg[S.ci[lane]] = FS_NONE; }
      continue;
    }
    // the keys
#pragma unroll
    for (int t = 0; t < kBatchW * kBatchH / 64; ++t) {
      const int w = (t * 64 + lane) / kBatchH, h = (t * 64 + lane) % kBatchH;
      if (h < L.H && S.ok[w]) S.key[w][h] = assemble_key(S.bal[w], h, L.B);
    }
    sync();
    // ---- B: bucket ranges, lane per (window, table) ----------------------------------------
#pragma unroll
    for (int t = 0; t < kBatchW * kBatchH / 64; ++t) {
      const int w = (t * 64 + lane) / kBatchH, h = (t * 64 + lane) % kBatchH;
      uint32_t e0 = 0, cnt_h = 0;
      if (h < L.H && S.ok[w]) {
        const uint32_t key = S.key[w][h];
        const uint32_t* o = L.boff + (size_t)h * nb1 + key;
        e0 = o[0];
        cnt_h = o[1] - e0;
      }
      // exclusive prefix inside the window's row of sixteen lanes
      uint32_t incl = cnt_h;
#pragma unroll
      for (int d = 1; d < kBatchH; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (h >= d) incl += up;
      }
      S.e0[w][h] = e0;
      S.pre[w][h] = incl - cnt_h;
      if (h == kBatchH - 1) S.vn[w] = incl;       // (the window's entries, until C needs vn)
    }
    sync();
    if (lane == 0) {
      uint32_t run = 0;
#pragma unroll
      for (int w = 0; w < kBatchW; ++w) { S.wbase[w] = run; run += S.vn[w]; S.vn[w] = 0; }
      S.wbase[kBatchW] = run;
    }
    sync();
    // ---- C: the members, 64 at a time -------------------------------------------------------
    const uint32_t total = (L.diag & 0x20000) ? 0u : S.wbase[kBatchW];      // (diagnostics: no members)
    if (L.diag & 0x80000) { if (lane == 0) atomicAdd(&st->max_rows, S.wbase[kBatchW]); }   // diagnostics: count them (printed by fs_search_corpus_end)
    for (uint32_t r0 = 0; r0 < total; r0 += 64) {
      const uint32_t j = r0 + lane;
      bool valid = false;
      uint32_t w = 0, s = 0;
      double d = 0.0;
      if (j < total) {
#pragma unroll
        for (int i = 1; i < kBatchW; ++i) w += S.wbase[i] <= j ? 1u : 0u;
        const uint32_t jw = j - S.wbase[w];
        uint32_t h = 0;                           // last table with pre[w][h] <= jw
#pragma unroll
        for (uint32_t step = kBatchH / 2; step > 0; step >>= 1)
          if (h + step < (uint32_t)L.H && S.pre[w][h + step] <= jw) h += step;
        s = L.bids[(size_t)h * L.W + S.e0[w][h] + (jw - S.pre[w][h])];
      }
      // A script window comes back once per table whose bucket it shares with the fan window --
      // a dozen times for a real neighbour -- and its distance is the same every time: one lane
      // of the round works it out for all that hold the same (window, script window) pair.  The
      // lanes agree on it through a small table in LDS (a lane that finds another pair's lane
      // in its slot works its own out).
      const uint32_t pair = s * (uint32_t)kBatchW + w;
      const uint32_t hslot = (pair * 0x9E3779B1u) >> 25;
      if (j < total) S.dh[hslot] = (uint32_t)lane;
      sync();
      const int leader = j < total ? (int)S.dh[hslot] : lane;
      const bool follow = (uint32_t)__shfl((int)pair, leader) == pair && leader != lane && j < total;
      if (j < total && !follow && !(L.diag & 0x40000))                  // (diagnostics: no distances)
        valid = window_distance_flat<N>(L, s, S.f[w], S.qf[w], S.ff[w], S.rff[w], &d) && d < L.thr;
      {
        const long long db = __double_as_longlong(d);
        const int lo = __shfl((int)(uint32_t)db, leader), hi = __shfl((int)(uint32_t)(db >> 32), leader);
        const int lv = __shfl((int)valid, leader);
        if (follow) { d = __longlong_as_double(((long long)hi << 32) | (uint32_t)lo); valid = lv != 0; }
      }
      // to the window's list, arrival order: the lanes of one window are consecutive
      const uint64_t vm = __ballot(valid);
      if (vm) {
        const uint32_t first = S.wbase[w] > r0 ? S.wbase[w] - r0 : 0u;        // the window's first lane of this round
        const uint64_t below = ((1ull << lane) - 1) & ~((1ull << first) - 1);
        const uint32_t slot = S.vn[w] + (uint32_t)__popcll(vm & below);
        if (valid && slot < (uint32_t)kBatchCap) { S.vs[w][slot] = s; S.vd[w][slot] = d; }
        sync();
        // the counts: the window's last valid lane of the round adds the round's number
        const uint32_t last_lane = min(63u, S.wbase[w + 1] - 1 - r0);
        const uint64_t mine = vm & (~0ull >> (63 - last_lane)) & ~((1ull << first) - 1);
        if (valid && (mine >> lane) == 1ull) S.vn[w] = slot + 1;
      }
      sync();
    }
    // ---- D: UniqueFilter, NearestFilter: eight lanes a window -----------------------------
    {
      const int w = lane >> 3, t = lane & 7;
      const uint32_t V = min(S.vn[w], (uint32_t)kBatchCap);
      const bool over = S.vn[w] > (uint32_t)kBatchCap;
      if (L.unique && !over) {
        for (uint32_t e = t; e < V; e += 8) {
          const uint32_t se = S.vs[w][e] & 0x7FFFFFFFu;
          bool dup = false;
          for (uint32_t x = 0; x < e; ++x) dup = dup || (S.vs[w][x] & 0x7FFFFFFFu) == se;
          if (dup) S.vs[w][e] = se | 0x80000000u;
        }
      }
      sync();
      uint32_t kept = 0;
      if (!over && (uint32_t)w < nw) {
        const uint32_t jj = S.jj[w];
        for (uint32_t e = t; e < V; e += 8) {
          const uint32_t se = S.vs[w][e];
          if (se & 0x80000000u) continue;
          ++kept;
          const double de = S.vd[w][e];
          uint32_t rank = 0;
          for (uint32_t x = 0; x < V; ++x) {
            const double dx = S.vd[w][x];
            rank += (!(S.vs[w][x] & 0x80000000u) && (dx < de || (dx == de && x < e))) ? 1u : 0u;
          }
          if (rank < nn) { mtop_s[(size_t)jj * nn + rank] = se; mtop_d[(size_t)jj * nn + rank] = de; }
        }
      }
      kept += (uint32_t)__shfl_xor((int)kept, 1);
      kept += (uint32_t)__shfl_xor((int)kept, 2);
      kept += (uint32_t)__shfl_xor((int)kept, 4);
      kept = min(kept, nn);
      if (t == 0 && (uint32_t)w < nw && !over) {
        const uint32_t i = S.ci[w];
        mcnt[S.jj[w]] = kept;
        cg[i] = kept ? FS_PENDING : FS_NONE;
        cw[i] = S.work[w];
        matches += kept;
      }
    }
    sync();
    // the crowded windows, a wave each (lsh_window with its scratch laid over the lists)
    for (uint32_t w = 0; w < nw; ++w) {
      if (S.vn[w] <= (uint32_t)kBatchCap) continue;             // (wave-uniform)
      uint8_t* raw = reinterpret_cast<uint8_t*>(&S.vd[0][0]);
      LshWaveLds X;
      X.bal = reinterpret_cast<uint64_t*>(raw);                  // 32 x 8
      X.top_d = reinterpret_cast<double*>(raw + 256);            // 64 x 8
      X.qf = reinterpret_cast<double*>(raw + 768);               // 16 x 8
      X.key = reinterpret_cast<uint32_t*>(raw + 896);            // 64 x 4
      X.top_s = X.key + 64; X.pre = X.key + 128; X.e0 = X.key + 192;
      X.f = X.key + 256; X.fs = X.key + 272;                     // 16 + 16
      X.n = reinterpret_cast<int*>(X.key + 288);
      X.lev = nullptr; X.la = nullptr; X.lb = nullptr;           // (deferred: no Levenshtein here)
      static_assert(896 + 4 * 292 <= sizeof(double) * kBatchW * kBatchCap + sizeof(uint32_t) * kBatchW * kBatchCap, "scratch");
      const uint32_t idv = lane < N ? S.f[w][lane] : 0u;
      const uint32_t i = S.ci[w], wk = S.work[w];
      sync();
      if (lane < N) { X.f[lane] = idv; X.fs[lane] = idv; }
      sync();
      fs_best b;
      const int cnt = lsh_window(c, L, g, X, st, &b, true);
      const uint32_t jj = S.jj[w];
      if (lane < cnt) {
        mtop_s[(size_t)jj * nn + lane] = X.top_s[lane];
        mtop_d[(size_t)jj * nn + lane] = X.top_d[lane];
      }
      if (lane == 0) {
        mcnt[jj] = (uint32_t)cnt;
        cg[i] = cnt ? FS_PENDING : FS_NONE;
        cw[i] = wk;
        matches += (uint32_t)cnt;
      }
      sync();
    }
  }
  uint32_t tot;
  block_excl_scan(matches, s_w32, &tot);
  if (threadIdx.x == 0) bmatch[blockIdx.x] += tot;       // (on top of k_lsh_sift's)
}

// ---- the pending windows without a bucket walk (round 5) --------------------------------------
// Every script window within the threshold of a pending window equals it in all slots but one --
// by vector ids where the table's c_max proves it (m_min = n - 1), by component ids on tables
// with near-synonyms -- so its n-gram sits in an exact map under one of the window's n one-slot-
// wildcard keys (build_emap).  What LSH finds of such an n-gram is decided by the keys alone:
// the tables in which its key is the window's (the script windows' keys are kept, d_skeys); all
// its occurrences share those buckets in ascending order; and everything beyond the threshold
// comes behind everything within it in NearestFilter's stable order, so it never changes the
// list.  A C2 batch on the clustered table walks 67 bucket members per pending window -- 18.9 M
// distances, nearly all of unrelated windows -- for lists that hold one script n-gram.
//   k_lsh_pkeys   the windows' 15 keys, eight windows per wave (k_lsh_batch's first stage)
//   k_lsh_enum    a LANE per window: the n map lookups, the n-gram's occurrences, keys and
//                 canonical distance, the list written in arrival order (table, occurrence)
// Windows with more than one such n-gram, a long chain in the map, or nn > 10 go to k_lsh_batch's
// bucket walk through a list of their own (a percent or two).
constexpr int kEnumNN = 10;               // NearestFilter sizes k_lsh_enum serves
constexpr int kEnumG = 4;                 // script n-grams one slot away from a window that it takes
struct alignas(16) PkeysLds {             // per wave
  uint64_t bal[kBatchW][kBatchBal];
  uint32_t f[kBatchW][FS_MAX_WINDOW];
  uint32_t pos[kBatchW], ok[kBatchW], work[kBatchW];
  float bnd[kBatchW];
};

template <int N>
__global__ __launch_bounds__(256) void k_lsh_pkeys(CorpusDev c, LshDev L, const uint32_t* __restrict__ cpos,
                                                   uint32_t cap, const uint32_t* __restrict__ pend,
                                                   const fs_status* st, uint32_t* __restrict__ pkeys,
                                                   uint32_t* __restrict__ pwork) {
  __shared__ PkeysLds s_b[4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  PkeysLds& S = s_b[wave];
  const uint32_t gw = blockIdx.x * 4 + wave, NWAVES = gridDim.x * 4;
  const uint32_t n_pend = min(st->lsh_pending, cap);
  auto sync = [] {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const uint32_t per = max(1u, min((uint32_t)kBatchW, (n_pend + NWAVES - 1) / NWAVES));
  for (uint32_t j0 = gw * per; j0 < n_pend; j0 += NWAVES * per) {
    const uint32_t nw = min(per, n_pend - j0);
    if (lane < kBatchW) {
      uint32_t ok = 0, w = FS_NONE;
      uint64_t p = 0;
      if ((uint32_t)lane < nw) {
        p = cpos[pend[j0 + lane]];
        if (p + N <= c.n_tok) {
          uint64_t work_end;
          const uint32_t wk = work_of_token(c, p, &work_end);
          if (p + N <= work_end) { ok = 1u; w = wk; }           // a window never crosses a work boundary
        }
      }
      S.pos[lane] = (uint32_t)p; S.ok[lane] = ok; S.work[lane] = w;
      S.bal[lane][(L.C + 63) >> 6] = 0;
    }
    sync();
#pragma unroll
    for (int t = 0; t < kBatchW * FS_MAX_WINDOW / 64; ++t) {      // lane per (window, slot)
      const int w = (t * 64 + lane) / FS_MAX_WINDOW, k = (t * 64 + lane) % FS_MAX_WINDOW;
      float am = 0.0f;
      uint32_t oov = 0;
      if (k < N && S.ok[w]) {
        const uint32_t id = c.tok[(uint64_t)S.pos[w] + k];
        S.f[w][k] = id;
        oov = id & FS_OOV_FLAG;
        if (!oov && L.atab32) am = L.amax[(size_t)k * L.V + id];
      }
#pragma unroll
      for (int d = 8; d > 0; d >>= 1) { am += __shfl_xor(am, d); oov |= (uint32_t)__shfl_xor((int)oov, d); }
      if (k == 0 && S.ok[w]) {
        S.bnd[w] = key_bound32(L, am, N);            // (no OOV id here: one addend a slot)
        if (oov || !L.atab32 || L.C > 256) S.ok[w] = 2u;
      }
    }
    sync();
    {
      const int col = 4 * lane;
      const int left = L.C - col;
      const uint32_t cmask = left >= 4 ? 0xFu : left > 0 ? (1u << left) - 1 : 0u;
      const int colc = left > 0 ? col : 0;
      for (uint32_t w = 0; w < nw; ++w) {
        if (S.ok[w] != 1u) continue;              // (wave-uniform)
        float4 r[N];
#pragma unroll
        for (int k = 0; k < N; ++k)
          r[k] = *reinterpret_cast<const float4*>(L.atab32 + ((size_t)k * L.V + S.f[w][k]) * L.Cp + colc);
        float4 acc = r[0];
#pragma unroll
        for (int k = 1; k < N; ++k) {
          acc.x = __fadd_rn(acc.x, r[k].x); acc.y = __fadd_rn(acc.y, r[k].y);
          acc.z = __fadd_rn(acc.z, r[k].z); acc.w = __fadd_rn(acc.w, r[k].w);
        }
        const float bnd = S.bnd[w];
        const uint32_t sure = (fabsf(acc.x) > bnd ? 1u : 0u) | (fabsf(acc.y) > bnd ? 2u : 0u) |
                              (fabsf(acc.z) > bnd ? 4u : 0u) | (fabsf(acc.w) > bnd ? 8u : 0u);
        if (__any((~sure & cmask) != 0u)) {
          if (lane == 0) S.ok[w] = 2u;            // a sign is not certain: float64 below
          continue;
        }
        uint32_t x = ((acc.x > 0.0f ? 1u : 0u) | (acc.y > 0.0f ? 2u : 0u) |
                      (acc.z > 0.0f ? 4u : 0u) | (acc.w > 0.0f ? 8u : 0u)) & cmask;
        x |= (uint32_t)__shfl_down((int)x, 1) << 4;
        x |= (uint32_t)__shfl_down((int)x, 2) << 8;
        x |= (uint32_t)__shfl_down((int)x, 4) << 16;
        uint32_t* pieces = reinterpret_cast<uint32_t*>(S.bal[w]);
        if ((lane & 7) == 0) pieces[lane >> 3] = x;
      }
    }
    sync();
    for (uint32_t w = 0; w < nw; ++w) {           // float64 keys where needed (rare)
      if (S.ok[w] != 2u) continue;
      for (int ch = 0; ch < (L.C + 63) >> 6; ++ch) {
        const int col = ch * 64 + lane;
        bool bit = false;
        if (col < L.C) {
          double acc = a_value(L, 0, S.f[w][0], col);
          for (int k = 1; k < N; ++k) acc = __dadd_rn(acc, a_value(L, k, S.f[w][k], col));
          bit = acc > 0.0;
        }
        const uint64_t b = __ballot(bit);
        if (lane == 0) S.bal[w][ch] = b;
      }
    }
    sync();
#pragma unroll
    for (int t = 0; t < kBatchW * kBatchH / 64; ++t) {
      const int w = (t * 64 + lane) / kBatchH, h = (t * 64 + lane) % kBatchH;
      if ((uint32_t)w < nw) pkeys[(size_t)(j0 + w) * kBatchH + h] = (h < L.H && S.ok[w]) ? assemble_key(S.bal[w], h, L.B) : 0u;
    }
    if (lane < kBatchW && (uint32_t)lane < nw) pwork[j0 + lane] = S.work[lane];
    sync();
  }
}

// CNT: with the counters of fs_index_lsh_counts (a form of its own: the kernel without them keeps
// its registers)
template <int N, bool CNT>
__global__ __launch_bounds__(256, 4) void k_lsh_enum(CorpusDev c, LshDev L, GramIndexDev g,
                                                  const uint32_t* __restrict__ cpos, uint32_t cap,
                                                  uint32_t* __restrict__ cg, uint32_t* __restrict__ cw,
                                                  uint32_t* __restrict__ bmatch, fs_status* st,
                                                  const uint32_t* __restrict__ pend,
                                                  const uint32_t* __restrict__ pkeys,
                                                  const uint32_t* __restrict__ pwork,
                                                  uint32_t* __restrict__ mcnt, uint32_t* __restrict__ mtop_s,
                                                  double* __restrict__ mtop_d,
                                                  uint32_t* __restrict__ left, uint32_t* __restrict__ n_left) {
  __shared__ uint32_t s_w32[4];
  const int lane = threadIdx.x & 63;
  const uint32_t n_pend = min(st->lsh_pending, cap);
  const uint32_t nn = (uint32_t)L.nn;
  uint32_t matches = 0;
  for (uint32_t j0 = blockIdx.x * 256; j0 < n_pend; j0 += gridDim.x * 256) {
    const uint32_t j = j0 + threadIdx.x;
    const bool live = j < n_pend;
    bool give_up = false;
    bool gu_fifth = false, gu_chain = false, reordered = false, cut = false;   // (for the counters)
    int deepest = 0;
    uint32_t work = FS_NONE, i = 0;
    uint64_t p = 0;
    if (live) { i = pend[j]; work = pwork[j]; p = cpos[i]; }
    const bool ok = live && work != FS_NONE;
    // ids (the buffers are padded: reading up to 12 is in bounds), the keys' ids, q
    uint32_t f[N], fc[N];
    double qf[N];
    {
      const uint4* a = reinterpret_cast<const uint4*>(c.tok + (ok ? p : 0));
      const uint4* b = reinterpret_cast<const uint4*>((L.emap_comp ? L.wild_tok : c.tok) + (ok ? p : 0));
#pragma unroll
      for (int q4 = 0; q4 < (N + 3) / 4; ++q4) {
        const uint4 x = a[q4], y = b[q4];
        const uint32_t xv[4] = {x.x, x.y, x.z, x.w}, yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * q4 + e < N) { f[4 * q4 + e] = xv[e]; fc[4 * q4 + e] = yv[e]; }
      }
    }
    uint32_t term[N], fold = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      term[k] = fs_rotl(fs_premix(fc[k]), fs_rot_of(N - 1 - k));
      fold ^= term[k];
      qf[k] = ok ? L.q[f[k]] : 0.0;             // (no OOV id on this path: the prefilters exclude them)
    }
    // the n map lookups, four requested together; the n-grams they name (kEnumG at most; a full
    // bucket's chain is followed twice)
    uint32_t gl[kEnumG];
    uint32_t gn = 0;
#pragma unroll
    for (int x = 0; x < kEnumG; ++x) gl[x] = FS_NONE;
    auto add_gram = [&](uint32_t gid) {
      bool seen = false;
#pragma unroll
      for (int x = 0; x < kEnumG; ++x) seen = seen || gl[x] == gid;
      if (seen) return;
      if (gn >= (uint32_t)kEnumG) { give_up = true; if (CNT) gu_fifth = true; return; }
#pragma unroll
      for (int x = 0; x < kEnumG; ++x) gl[x] = gn == (uint32_t)x ? gid : gl[x];
      ++gn;
    };
#pragma unroll
    for (int k0 = 0; k0 < N; k0 += 4) {
      uint4 ba[4], bb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k0 + u < N) {
          const uint32_t h = fs_wild_key(fold, term[k0 + u], k0 + u);
          const uint4* bp = reinterpret_cast<const uint4*>(L.emap + 4 * (size_t)fs_wmap_slot(h, L.log2_emap));
          ba[u] = bp[0]; bb[u] = bp[1];
        }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k0 + u < N) {
          const uint32_t h = fs_wild_key(fold, term[k0 + u], k0 + u);
          uint4 a = ba[u], b = bb[u];
          uint32_t bkt = fs_wmap_slot(h, L.log2_emap);
          for (int probe = 0;; ++probe) {
            const uint32_t key[4] = {a.x, a.z, b.x, b.z}, val[4] = {a.y, a.w, b.y, b.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (val[e] && key[e] == h && ok) add_gram(val[e] - 1);
            if (CNT) deepest = max(deepest, probe);               // (the chain's buckets read behind the first)
            if (!val[3] || !ok) break;            // (not full: nothing has spilt past it)
            if (probe == 2) { give_up = true; if (CNT) gu_chain = true; break; }
            bkt = (bkt + 1) & ((1u << L.log2_emap) - 1u);
            const uint4* bp = reinterpret_cast<const uint4*>(L.emap + 4 * (size_t)bkt);
            a = bp[0]; b = bp[1];
          }
        }
    }
    if (!ok) give_up = false;
    // per n-gram: the canonical distance to its first window (window_distance_flat's arithmetic,
    // the fan side in registers) and the tables that hold both in one bucket
    double gd[kEnumG];
    uint32_t gt[kEnumG];
#pragma unroll
    for (int x = 0; x < kEnumG; ++x) { gd[x] = 0.0; gt[x] = 0; }
    if (ok && !give_up && gn) {
      double ff = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) ff = __dadd_rn(ff, qf[k]);
      const double rff = __dsqrt_rn(ff);
      uint32_t mine[kBatchH];
#pragma unroll
      for (int q4 = 0; q4 < kBatchH / 4; ++q4) {
        const uint4 m = reinterpret_cast<const uint4*>(pkeys + (size_t)j * kBatchH)[q4];
        mine[4 * q4] = m.x; mine[4 * q4 + 1] = m.y; mine[4 * q4 + 2] = m.z; mine[4 * q4 + 3] = m.w;
      }
      for (uint32_t gi = 0; gi < gn; ++gi) {
        uint32_t gid = gl[0];
#pragma unroll
        for (int x = 1; x < kEnumG; ++x) gid = gi == (uint32_t)x ? gl[x] : gid;
        if (gid >= g.n_grams) continue;           // (cannot happen: the map holds gram ids)
        const uint32_t s0 = g.gpos[(size_t)gid * nn];
        uint32_t tables = 0;
#pragma unroll
        for (int h = 0; h < kBatchH; ++h)
          tables |= (h < L.H && L.skeys[(size_t)s0 * L.H + h] == mine[h]) ? 1u << h : 0u;
        const fs_swin sw = L.sw[s0];
        uint4 rec[N];
#pragma unroll
        for (int k = 0; k < N; ++k) rec[k] = *reinterpret_cast<const uint4*>(L.spos + s0 + k);
        int same = 0;
        uint32_t diff = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const bool eq = rec[k].w == f[k];
          same += eq;
          diff |= eq ? 0u : 1u << k;
        }
        double d = 0.0;
        bool v = !(L.m_min > 0 && same < L.m_min);
        if (v) {
          const double norm = __dmul_rn(sw.rss, rff);
          double sf;
          if (same == N) {
            sf = sw.ss;
          } else {
            double gk[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
              gk[k] = qf[k];
              if (diff >> k & 1u) gk[k] = L.gtab[(size_t)(int32_t)rec[k].z * L.V + f[k]];
            }
            sf = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) sf = __dadd_rn(sf, gk[k]);
          }
          d = __dsub_rn(1.0, __ddiv_rn(sf, norm));
          v = d == d && d < L.thr;
        }
        if (!v) tables = 0;
        if (L.unique && tables) tables &= 0u - tables;           // a script window counts where it arrives first
#pragma unroll
        for (int x = 0; x < kEnumG; ++x)
          if (gi == (uint32_t)x) { gd[x] = d; gt[x] = tables; }
      }
    }
    // NearestFilter's order: by distance, the n-grams one after the other (entries of one n-gram
    // share its distance and are in arrival order).  Two n-grams at exactly the same distance
    // would interleave by arrival: left to the bucket walk.
    auto cswap = [&](int a, int b) {
      const bool sw2 = (gt[b] != 0 && (gt[a] == 0 || gd[b] < gd[a]));
      if (CNT) reordered = reordered || (sw2 && gt[a] != 0);
      const double da = gd[a], db = gd[b];
      const uint32_t ta = gt[a], tb2 = gt[b], ga = gl[a], gb = gl[b];
      gd[a] = sw2 ? db : da; gd[b] = sw2 ? da : db;
      gt[a] = sw2 ? tb2 : ta; gt[b] = sw2 ? ta : tb2;
      gl[a] = sw2 ? gb : ga; gl[b] = sw2 ? ga : gb;
    };
    static_assert(kEnumG == 4, "a sorting network of four");
    cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
    bool tie = false;
#pragma unroll
    for (int x = 0; x + 1 < kEnumG; ++x)
      if (gt[x] && gt[x + 1] && gd[x] == gd[x + 1]) { give_up = true; if (CNT) tie = true; }
    uint32_t made = 0;
    if (ok && !give_up) {
      const size_t jj = (size_t)j * nn;
#pragma unroll
      for (int x = 0; x < kEnumG; ++x) {
        if (CNT && gt[x] && made >= nn) cut = true;
        if (!gt[x] || made >= nn) continue;
        const uint32_t gid = gl[x], occ = g.gcnt[gid];
        uint32_t o[kEnumNN];
#pragma unroll
        for (int r = 0; r < kEnumNN; ++r) o[r] = (uint32_t)r < nn ? g.gpos[(size_t)gid * nn + r] : 0u;
        uint32_t tb = gt[x], r = 0;
#pragma unroll
        for (int e = 0; e < kEnumNN; ++e)
          if (tb && made < nn) {
            uint32_t sel = o[0];
#pragma unroll
            for (int y = 1; y < kEnumNN; ++y) sel = r == (uint32_t)y ? o[y] : sel;
            mtop_s[jj + made] = sel;
            mtop_d[jj + made] = gd[x];
            ++made;
            if (++r == occ) { r = 0; tb &= tb - 1; }
          }
        if (CNT && tb) cut = true;                // (entries of this n-gram beyond the N kept)
      }
    }
    if (CNT) {                                    // diagnostics (fs_index_lsh_counts)
      const bool listed = ok && !give_up;
      uint32_t within = 0;
#pragma unroll
      for (int x = 0; x < kEnumG; ++x) within += gt[x] ? 1u : 0u;
      lsh_count(L.lsh_cnt, kCntEnumListed1, listed && within == 1);
      lsh_count(L.lsh_cnt, kCntEnumListed2, listed && within == 2);
      lsh_count(L.lsh_cnt, kCntEnumListed3, listed && within == 3);
      lsh_count(L.lsh_cnt, kCntEnumListed4, listed && within == 4);
      lsh_count(L.lsh_cnt, kCntEnumReordered, listed && reordered);
      lsh_count(L.lsh_cnt, kCntEnumCut, listed && cut);
      lsh_count(L.lsh_cnt, kCntEnumChainOnce, ok && !gu_chain && deepest == 1);
      lsh_count(L.lsh_cnt, kCntEnumChainTwice, ok && !gu_chain && deepest == 2);
      lsh_count(L.lsh_cnt, kCntEnumGiveUpFifth, ok && gu_fifth);
      lsh_count(L.lsh_cnt, kCntEnumGiveUpChain, ok && gu_chain);
      lsh_count(L.lsh_cnt, kCntEnumGiveUpTie, ok && tie);
    }
    if (live && !give_up) {
      mcnt[j] = made;
      cg[i] = made ? FS_PENDING : FS_NONE;
      if (ok) cw[i] = work;
      matches += made;
    }
    // the windows left to the bucket walk, one addition per wave
    const uint64_t gm = __ballot(live && give_up);
    if (gm) {
      uint32_t base = 0;
      if (lane == 0) base = atomicAdd(n_left, (uint32_t)__popcll(gm));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, 0);
      if (live && give_up)
        left[base + __builtin_amdgcn_mbcnt_hi((uint32_t)(gm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)gm, 0u))] = j;
    }
  }
  uint32_t tot;
  block_excl_scan(matches, s_w32, &tot);
  if (threadIdx.x == 0) bmatch[blockIdx.x] += tot;       // (on top of k_lsh_sift's)
}

// The Levenshtein distances of the matches k_lsh_verify<true> kept, and the record of every
// pending window: a lane per (window, rank) pair -- lev_lane, Myers' recurrence on one lane's
// registers against the script window's bit planes, where k_lsh_verify ran it as a wave per
// pair on the scalar unit (a ballot per column and ~20 scalar instructions: the CU's one
// scalar unit was busy more than half of that kernel's time).  A workgroup takes 128 windows at
// a time (a pair is ~4 us of one lane's time whatever else runs: the fewer rounds of pairs a
// workgroup has to make, the better -- 128 windows are one round of its 256 lanes unless they
// keep two matches each): prefix sum of their match counts, the pairs dealt out evenly over
// the threads (the window of a pair by binary search in LDS), the distances through LDS, then a
// lane per window takes the first minimum of dist * lev in rank order (search.py:224-225).
constexpr int kLevMaxN = 16;            // NearestFilter sizes this form serves (the default is 10)
constexpr uint32_t kLevWin = 128;       // windows per workgroup and step
__global__ __launch_bounds__(256) void k_lsh_lev(CorpusDev c, LshDev L, GramIndexDev g, StrFast F,
                                                 const uint32_t* __restrict__ cpos, uint32_t cap,
                                                 const uint32_t* __restrict__ pend,
                                                 const uint32_t* __restrict__ mcnt,
                                                 const uint32_t* __restrict__ mtop_s,
                                                 const double* __restrict__ mtop_d,
                                                 uint32_t* __restrict__ cg, fs_best* __restrict__ cbest,
                                                 fs_status* st) {
  __shared__ uint32_t s_w32[4];
  __shared__ uint32_t s_pref[257];
  __shared__ uint32_t s_lev[kLevWin * kLevMaxN];
  __shared__ uint8_t s_first[kLevWin * kLevMaxN], s_dr[kLevWin * kLevMaxN];
  const uint32_t n_pend = min(st->lsh_pending, cap);
  const uint32_t nn = (uint32_t)L.nn;
  for (uint32_t j0 = blockIdx.x * kLevWin; j0 < n_pend; j0 += gridDim.x * kLevWin) {
    const uint32_t j = j0 + threadIdx.x;
    const uint32_t cnt = (threadIdx.x < kLevWin && j < n_pend) ? mcnt[j] : 0u;
    // Without the UniqueFilter a script window is kept once per table that found it, and the
    // copies' Levenshtein distance is the one number: a pair per DISTINCT script window of
    // the list (first[r]: the first rank with rank r's window; dr[k]: rank of the k-th distinct
    // one), up to ten times fewer pairs
    uint32_t dcnt = 0;
    for (uint32_t r = 0; r < cnt; ++r) {
      const uint32_t sr = mtop_s[(size_t)j * nn + r];
      uint32_t fr = r;
      for (uint32_t x = 0; x < r; ++x)
        if (mtop_s[(size_t)j * nn + x] == sr) { fr = x; break; }
      s_first[threadIdx.x * kLevMaxN + r] = (uint8_t)fr;
      if (fr == r) s_dr[threadIdx.x * kLevMaxN + dcnt++] = (uint8_t)r;
    }
    uint32_t total;
    const uint32_t base = block_excl_scan(dcnt, s_w32, &total);
    s_pref[threadIdx.x] = base;
    if (threadIdx.x == 255) s_pref[256] = total;
    __syncthreads();
    for (uint32_t q0 = 0; q0 < total; q0 += 256) {
      const uint32_t q = q0 + threadIdx.x;
      if (q < total) {
        uint32_t lo = 0, hi = 256;               // s_pref[lo] <= q < s_pref[hi]
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (s_pref[mid] <= q) lo = mid; else hi = mid;
        }
        const uint32_t r = s_dr[lo * kLevMaxN + (q - s_pref[lo])], jj = j0 + lo;
        const uint32_t s = mtop_s[(size_t)jj * nn + r];
        const uint64_t p = cpos[pend[jj]];
        uint32_t lv = FS_NONE;
        if (L.selflev) {
          // a match with the same id in every slot has the strings of the script window's own
          // ids: its distance was computed once per string table (k_selflev)
          Ids16 u, f;
          load_ids(L.stok + s, L.n, &u);
          load_ids(c.tok + p, L.n, &f);
          bool same = true;
#pragma unroll
          for (int k = 0; k < FS_MAX_WINDOW; ++k)
            if (k < L.n) same = same && u.v[k] == f.v[k];
          if (same) lv = L.selflev[s];
        }
        if (lv == FS_NONE) {
          Ids16 sid;
          load_ids((c.str ? c.str : c.tok) + p, L.n, &sid);
          bool bad = false;
#pragma unroll
          for (int k = 0; k < FS_MAX_WINDOW; ++k)
            if (k < L.n) bad = bad || sid.v[k] >= c.n_str;
          if (bad) { st->bad_string = 1; lv = 0; }
          else lv = lev_lane_ids(g, c, F, s, sid, st);
        }
        s_lev[lo * nn + r] = lv;
      }
    }
    __syncthreads();
    if (cnt) {
      fs_best b;
      b.pad = 0.0;
      for (uint32_t r = 0; r < cnt; ++r) {          // first minimum of dist * lev in rank order
        const double d = mtop_d[(size_t)j * nn + r];
        const uint32_t lv = s_lev[threadIdx.x * nn + s_first[threadIdx.x * kLevMaxN + r]];
        const double comb = __dmul_rn(d, (double)lv);
        if (r == 0 || comb < b.comb) {
          b.s = mtop_s[(size_t)j * nn + r]; b.lev = lv; b.dist = d; b.comb = comb;
        }
      }
      const uint32_t i = pend[j];
      cbest[i] = b;
      cg[i] = 0;
    }
    __syncthreads();
  }
}

}  // namespace

// ---- host side -----------------------------------------------------------------

// the strings of the batch's table against every script n-gram, once per string table; the
// status block of lane 0 collects string errors (bad_string, lev_overflow) for the caller
int fs_launch_lsh_gramtab(fs_index* ix, fs_corpus* c, hipStream_t s) {
  if (!ix->n_grams) return FS_OK;
  LshDev L = lsh_dev(ix);
  if (c->selflev_ready) L.selflev = c->d_selflev.p;
  FS_TRY(c->d_gramtab_best.reserve(4 * (size_t)ix->n_grams));
  FS_TRY(c->d_gramtab_cnt.reserve(ix->n_grams));
  const uint32_t blocks = (ix->n_grams + 3) / 4;
  hipLaunchKernelGGL(k_lsh_gramtab, dim3(blocks > kNB ? kNB : blocks), dim3(256), 0, s, c->dev(), L,
                     ix->gram_dev(), c->d_gramtab_best.p, c->d_gramtab_cnt.p, ix->cur->d_status.p);
  FS_HIP(hipGetLastError());
  return FS_OK;
}

// The wildcard-key filter that stands in front of the LSH work of a search of `c` (nullptr: none),
// and the ids its keys are made of (nullptr: the vector ids).
void fs_lsh_wild_of(const fs_index* ix, const fs_corpus* c, const uint32_t** wild, int* log2_wild,
                    const uint32_t** wild_tok) {
  *wild = nullptr; *log2_wild = 0; *wild_tok = nullptr;
  // tables with near-synonyms: the wildcard keys over component ids (no one-slot map: a
  // neighbour may differ from the window in every vector id)
  if (fs_lsh_prefilter_mode(ix, c) == 2 && ix->sw.lsh_wild) {
    *wild = ix->d_wildc.p;
    *log2_wild = ix->log2_wildc;
    *wild_tok = c->d_ctok.p;
  }
  // at most one slot may differ and no OOV id anywhere: the wildcard-key filter applies
  if (ix->sw.lsh_wild && ix->d_wild.p && !c->has_oov && !ix->script_oov &&
      (int)ix->cfg.window_size - ix->lsh_m_min == 1) {
    *wild = ix->d_wild.p;
    *log2_wild = ix->log2_wild;
    *wild_tok = nullptr;
  }
}

// one resident set of workgroups each (the kernels loop over their work and are bound by the
// latency of dependent loads: a second, partial round of workgroups costs a whole round's time)
uint32_t lsh_resident_blocks(const fs_index* ix, const void* kern) {
  if (ix->sw.lsh_full_grid) return kNB;
  static std::mutex mu;
  static std::vector<std::pair<const void*, int>> seen;      // workgroups per CU, asked once per kernel
  int per_cu = 0;
  {
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : seen)
      if (e.first == kern) per_cu = e.second;
    if (!per_cu) {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, 0) != hipSuccess || per_cu < 1)
        per_cu = -1;
      seen.push_back({kern, per_cu});
    }
  }
  return per_cu < 1 ? (uint32_t)kNB : std::min<uint32_t>(kNB, ix->num_cu * (uint32_t)per_cu);
}

// the pending windows (fs_launch_lsh_verify, behind the sift)
static int lsh_launch_pending(fs_index* ix, fs_corpus* c, const LshDev& L, uint32_t ccap, hipStream_t s) {
  fs_status* st = ix->cur->d_status.p;
  const NSrc nc{&st->n_cands, 1, ccap, 0};
  // the kept matches' Levenshtein distances a lane per match (k_lsh_lev) where the script
  // windows' bit planes and the string table's records exist; else a wave per match inside
  // k_lsh_verify
  // (a launch of its own costs ~20 us whatever it finds to do -- the chain of loads in front of a
  // pair and the pair itself, 4 us of one lane's time: worth it from some thousands of pending
  // windows on, which the lane's last search tells; FS_LSH_LEV_LANE=2: always)
  const bool defer = ix->sw.lsh_lev_lane && ix->sw.str_fast && ix->strfast_ok && c->strrec_ready &&
                     L.nn <= kLevMaxN && (ix->cur->pend_hint >= (uint32_t)ix->sw.lsh_defer_min || ix->sw.lsh_lev_lane == 2);
  if (defer) {
    FS_TRY(ix->cur->w_mcnt.reserve(ccap));
    FS_TRY(ix->cur->w_mtop_s.reserve((size_t)ccap * L.nn));
    FS_TRY(ix->cur->w_mtop_d.reserve((size_t)ccap * L.nn));
  }
  // the pending windows eight at a time per wave (k_lsh_batch) where the kept matches' Levenshtein
  // distances are k_lsh_lev's anyway; a wave per window (k_lsh_verify) otherwise.  Where the script
  // n-grams one slot away can be enumerated (L.emap), k_lsh_pkeys + k_lsh_enum take the windows
  // first and k_lsh_batch only what they leave.
  typedef void (*BatchFn)(CorpusDev, LshDev, GramIndexDev, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                          fs_status*, const uint32_t*, uint32_t*, uint32_t*, double*, const uint32_t*, const uint32_t*);
  typedef void (*PkeysFn)(CorpusDev, LshDev, const uint32_t*, uint32_t, const uint32_t*, const fs_status*, uint32_t*, uint32_t*);
  typedef void (*EnumFn)(CorpusDev, LshDev, GramIndexDev, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                         fs_status*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, double*,
                         uint32_t*, uint32_t*);
  BatchFn batch = nullptr;
  PkeysFn pkeys = nullptr;
  EnumFn enumk = nullptr;
  if (defer && ix->sw.lsh_batch && L.H <= kBatchH && L.nn <= 48 && !L.serial_neighbours && !(L.diag & 0xFFFF))
    switch (L.n) {
#define FS_B(N) case N: batch = k_lsh_batch<N>; pkeys = k_lsh_pkeys<N>; \
                        enumk = L.lsh_cnt ? k_lsh_enum<N, true> : k_lsh_enum<N, false>; break
      FS_B(6); FS_B(7); FS_B(8); FS_B(9); FS_B(10); FS_B(12);
#undef FS_B
      default: break;
    }
  if (batch) {
    const bool enumerate = L.emap && L.skeys && L.spos && L.gtab && L.nn <= kEnumNN;
    const uint32_t* left = nullptr;
    const uint32_t* n_left = nullptr;
    if (enumerate) {
      FS_TRY(ix->cur->w_pkeys.reserve((size_t)ccap * kBatchH));
      FS_TRY(ix->cur->w_pwork.reserve(ccap));
      FS_TRY(ix->cur->w_left.reserve(ccap));
      const uint32_t kb = lsh_resident_blocks(ix, reinterpret_cast<const void*>(pkeys));
      hipLaunchKernelGGL(pkeys, dim3(kb), dim3(256), 0, s, c->dev(), L, ix->cur->w_cpos.p, ccap, ix->cur->w_pend.p,
                         st, ix->cur->w_pkeys.p, ix->cur->w_pwork.p);
      if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_pkeys");
      const uint32_t eb = lsh_resident_blocks(ix, reinterpret_cast<const void*>(enumk));
      hipLaunchKernelGGL(enumk, dim3(eb), dim3(256), 0, s, c->dev(), L, ix->gram_dev(), ix->cur->w_cpos.p, ccap,
                         ix->cur->w_cg.p, ix->cur->w_cw.p, ix->cur->w_bsum.p + kNB, st, ix->cur->w_pend.p,
                         ix->cur->w_pkeys.p, ix->cur->w_pwork.p, ix->cur->w_mcnt.p, ix->cur->w_mtop_s.p,
                         ix->cur->w_mtop_d.p, ix->cur->w_left.p, &st->n_hits);
      if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_enum");
      left = ix->cur->w_left.p;
      n_left = &st->n_hits;
    }
    const uint32_t blocks = lsh_resident_blocks(ix, reinterpret_cast<const void*>(batch));
    hipLaunchKernelGGL(batch, dim3(blocks), dim3(256), 0, s, c->dev(), L, ix->gram_dev(),
                       ix->cur->w_cpos.p, ccap, ix->cur->w_cg.p, ix->cur->w_cw.p, ix->cur->w_bsum.p + kNB, st,
                       ix->cur->w_pend.p, ix->cur->w_mcnt.p, ix->cur->w_mtop_s.p, ix->cur->w_mtop_d.p, left, n_left);
    if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_batch");
  } else {
  auto verify = defer ? k_lsh_verify<true> : k_lsh_verify<false>;
  const uint32_t verify_blocks = lsh_resident_blocks(ix, reinterpret_cast<const void*>(verify));
  hipLaunchKernelGGL(verify, dim3(verify_blocks), dim3(256), 0, s, c->dev(), L, ix->gram_dev(),
                     ix->cur->w_cpos.p, nc, ix->cur->w_cg.p, ix->cur->w_cw.p, ix->cur->w_cbest.p,
                     ix->cur->w_bsum.p + kNB, st, ix->cur->w_pend.p, ix->cur->w_mcnt.p,
                     ix->cur->w_mtop_s.p, ix->cur->w_mtop_d.p);
  if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_verify");
  }
  if (defer) {
    const StrFast F{ix->d_pat.p, ix->d_clsmap.p, ix->n_cls, ix->str_punct, c->d_strrec.p};
    const uint32_t lev_blocks = lsh_resident_blocks(ix, reinterpret_cast<const void*>(k_lsh_lev));
    hipLaunchKernelGGL(k_lsh_lev, dim3(lev_blocks), dim3(256), 0, s, c->dev(), L, ix->gram_dev(), F,
                       ix->cur->w_cpos.p, ccap, ix->cur->w_pend.p, ix->cur->w_mcnt.p,
                       ix->cur->w_mtop_s.p, ix->cur->w_mtop_d.p, ix->cur->w_cg.p, ix->cur->w_cbest.p, st);
    if (ix->prof.on) fs_prof_mark(ix, s, "k_lsh_lev");
  }
  return FS_OK;
}

// near: the candidates come from k_near_sift's lists (the wildcard filter applied):
// k_lsh_sift2 numbers them and takes the second stage, instead of k_lsh_sift over k_expand's list
int fs_launch_lsh_verify(fs_index* ix, fs_corpus* c, uint32_t ccap, hipStream_t s, const fs_near_lists* near) {
  LshDev L = lsh_dev(ix);
  if (c->selflev_ready && !c->has_str) L.selflev = c->d_selflev.p;
  // the wildcard-key filter of this search, if any (fs_lsh_wild_of)
  fs_lsh_wild_of(ix, c, &L.wild, &L.log2_wild, &L.wild_tok);
  // every neighbour within the threshold equals the window in all slots but one (by vector
  // ids, or by component ids): the exact map enumerates them, no bucket is walked (k_lsh_batch)
  if (ix->sw.lsh_emap && L.wild) {
    if (L.wild_tok && ix->d_emapc.p && ix->log2_emapc) {
      L.emap = reinterpret_cast<const uint2*>(ix->d_emapc.p); L.log2_emap = ix->log2_emapc; L.emap_comp = 1;
    } else if (!L.wild_tok && ix->d_emap.p && ix->log2_emap) {
      L.emap = reinterpret_cast<const uint2*>(ix->d_emap.p); L.log2_emap = ix->log2_emap; L.emap_comp = 0;
    }
  }
  if (L.wild && !L.wild_tok) {
    // A one-slot neighbour has cosine (n - 1 + c) / n with c the cosine of the two differing
    // vectors: within the threshold iff c > 1 - n * thr.  At n = 8 (c > 0.2) nearly every such
    // window ends in k_lsh_sift; at n = 10 (c > 0) half of them are real neighbours and stay
    // pending, the other half still ends there.
    if (ix->sw.lsh_wmap && ix->d_wmap.p) {
      L.wmap = reinterpret_cast<const uint2*>(ix->d_wmap.p);
      L.log2_wmap = ix->log2_wmap;
    }
  }
  FS_TRY(ix->cur->w_pend.reserve(ccap));
  FS_TRY(lsh_launch_sift(ix, c, L, ccap, s, near));
  FS_TRY(lsh_launch_pending(ix, c, L, ccap, s));
  FS_HIP(hipGetLastError());
  return FS_OK;
}
