// fs_lsh.h -- what the units of the general (LSH) pipeline share (fs_lsh.hip describes it):
//   fs_lsh_build.hip    the index: projection tables, pair table, script window keys and their
//                       CSR buckets, the prefilters' filters and maps, the share rule's index side
//   fs_lsh_share.hip    which windows have a script window within the threshold in a shared bucket:
//                       k_lsh_scan, and the share rule in front of it or in its place
//   fs_lsh_sift.hip     a lane per flagged window, where at most one slot may differ: most end there
//   fs_lsh.hip          the windows that are left (pending): neighbour lists, Levenshtein
//                       distances, best rank -> per-candidate record for k_rows
// LshDev (what every kernel gets of the index), and only those device helpers and constants that
// two or more units use; a helper with one user lives in that user's file.
#pragma once

#include "fs_device.h"

struct LshDev {
  const double* atab;      // [n][V][C]
  const double* nt;        // [n][D][C] normals transposed
  const uint32_t* boff;    // [H][2^B + 1]
  const uint32_t* bids;    // [H][W]
  const double* ss;        // [W] sum of q over script window
  const fs_swin* sw;       // [W] first-slot record per script window
  const double* q;         // [V]
  const float* emb;        // [V][D]
  const uint32_t* stok;    // script vector ids
  const float* atab32;     // [n][V][Cp] float32 copy of atab (rows padded to Cp = 4*ceil(C/4)
                           // floats with zeros, 16-byte aligned), or nullptr
  const float* amax;       // [n][V] >= max_c |atab[k][v][c]|
  const float* nt32;       // [n][D][Cp] float32 copy of nt (rows padded like atab32): the projection row of an
                           // out-of-vocabulary vector is the sum of the rows of its (up to three) hot positions
  const float* ntmax;      // [n][D] >= max_c |nt[k][d][c]|
  float bound_scale;       // n * 2^-22 (times a test factor)
  float bound_abs;         // 2^-149 (times the same factor): key_bound32's absolute term per addend
  int m_min;               // fewer id-identical slots than this cannot reach the threshold
  int diag;                // diagnostics: 1 = skip candidate walk, 2 = skip key computation,
                           // 3 = walk the buckets but skip the distances
  int serial_neighbours;   // FS_LSH_SERIAL=1: k_lsh_verify walks the buckets on one lane (cross-check)
  const double* gtab;      // [n_srow][V] g(script row, table row), or nullptr
  const int32_t* sidx;     // [V] row of gtab for a table id, -1 if not a script word
  const uint2* emap;       // one-slot-wildcard keys (over the vector ids, or the component ids: emap_comp) -> distinct
                           // script n-gram: 2^log2_emap buckets of four {key, gram + 1} (k_lsh_batch), or nullptr
  int log2_emap, emap_comp;
  const uint32_t* skeys;   // [W][H] LSH keys of the script windows
  const fs_spos* spos;     // [n_script] {q, pair-table row, id} of every script token (k_spos), or nullptr
  const uint32_t* selflev; // [W] Levenshtein of script window w against the strings of its own ids for
                           // this batch's string table (FS_NONE: compute), or nullptr
  const uint32_t* wild;    // one-slot-wildcard keys of the script windows (fs_hash.h), or nullptr
  int log2_wild;
  const uint32_t* wild_tok;// the ids the keys are made of: nullptr = the vector ids, else the
                           // component ids of the batch's tokens (tables with near-synonyms)
  const uint2* wmap;       // the same keys as an exact map: 2^log2_wmap buckets of four {key, script window + 1}, or nullptr
  int log2_wmap;
  // the share rule (fs_build_share): component ids under the angular relation of the table's vectors and
  // of the script's tokens, the script windows' subset keys, and its constants
  const uint32_t* compa;   // [V], or nullptr: the rule is not in use
  const uint64_t* ssig;    // [W] the script windows' component signatures (share_pair_possible)
  const uint32_t* sharef;  // 2^log2_sharef filter words
  const uint2* smap;       // the same keys as an exact map: 2^log2_smap buckets of four {key, list} (k_share_scan)
  const uint4* slists;     // the lists of the map: a list's length (.x), then its script windows with their signature words
                           // {window, word's low half, high half, 0} (the map names the first of those)
  int log2_smap;
  int log2_sharef, share_flags;
  unsigned long long* share_cnt;   // diagnostics (FS_SHARE_COUNT=1): k_share_scan's counters, or nullptr
  const uint2* oovmap;     // the script's out-of-vocabulary vectors (share_comp): 2^log2_oovmap {key, component}, or nullptr
  int log2_oovmap;
  float share_lim;         // <= 1 - phi: the share of a window's squared norm its near slots must hold
  double share_scale;      // squared norms as integers: floor(q * share_scale) <= 2^20
  double share_phi, share_tau, share_gamma;
  uint32_t V, W;
  int n, H, B, D, C, Cp, nn, unique;
  double thr, cmax;
  unsigned long long* lsh_cnt;     // diagnostics (FS_LSH_COUNT=1): which branch of the one-slot maps a window took
                                   // (LshCount below; k_lsh_sift*, k_lsh_enum), or nullptr
};

// shared by the units, not exported from the library (fs_internal.h's functions are the ones
// other files call)
#define FS_LSH_LOCAL __attribute__((visibility("hidden")))

FS_LSH_LOCAL LshDev lsh_dev(const fs_index* ix);                                   // fs_lsh_build.hip
// workgroups for a kernel that loops over its work: one resident set, asked once per kernel
// (FS_LSH_FULL_GRID=1: kNB)
FS_LSH_LOCAL uint32_t lsh_resident_blocks(const fs_index* ix, const void* kern);   // fs_lsh.hip
// the first half of fs_launch_lsh_verify (fs_lsh.hip)
FS_LSH_LOCAL int lsh_launch_sift(fs_index* ix, fs_corpus* c, const LshDev& L, uint32_t ccap, hipStream_t s,
                                 const fs_near_lists* near);                       // fs_lsh_sift.hip

// cg[i] of a window that k_lsh_sift leaves to the kernels of fs_lsh.hip
constexpr uint32_t FS_PENDING = 0xFFFFFFFEu;
// component id of a fan token that counts as agreeing with anything (share_comp, fs_build_share)
#define FS_WILD 0xFFFFFFFEu
// The counters behind LshDev::lsh_cnt, in the order fs_index_lsh_counts returns them: windows by
// the branch they took in sift_stage2 (each window in one of the first eight at most: the reasons
// to stay pending in the order the code asks them -- a full bucket, more than two n-grams, a
// distance) and in k_lsh_enum (listed windows by their number of n-grams within the threshold;
// a window may give up for more than one reason and counts under each).
enum LshCount {
  kCntRecordNeighbours = 0, kCntRecordAlone, kCntWmapEnded0, kCntWmapEnded1, kCntWmapEnded2,
  kCntWmapPendingDistance, kCntWmapPendingMany, kCntWmapPendingFull,
  kCntEnumListed1, kCntEnumListed2, kCntEnumListed3, kCntEnumListed4, kCntEnumReordered, kCntEnumCut,
  kCntEnumChainOnce, kCntEnumChainTwice, kCntEnumGiveUpFifth, kCntEnumGiveUpChain, kCntEnumGiveUpTie,
  kCntLsh                                    // (their number; FS_LSH_COUNTERS of the header holds room for them)
};

// (an anonymous namespace in a header: every unit gets its own copy, inlined into its kernels,
// and nothing is exported; a unit uses some of these, not all)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
namespace {

// diagnostics: the lanes with `on` (of those that are active here) add to counter `which`, one
// addition per wave
__device__ __forceinline__ void lsh_count(unsigned long long* cnt, int which, bool on) {
  const unsigned long long b = __ballot(on);
  if (on && (int)(threadIdx.x & 63) == __ffsll(b) - 1) atomicAdd(cnt + which, (unsigned long long)__popcll(b));
}

// ---- canonical per-token quantities ------------------------------------------

__device__ __forceinline__ void oov_hot(uint32_t id, int D, uint32_t* a, uint32_t* b, uint32_t* c) {
  const uint32_t code = id & ~FS_OOV_FLAG;
  *c = code % D; *b = (code / D) % D; *a = code / ((uint32_t)D * D);
}

// A[k][id][c]
__device__ __forceinline__ double a_value(const LshDev& L, int k, uint32_t id, int c) {
  if (!(id & FS_OOV_FLAG)) return L.atab[((size_t)k * L.V + id) * L.C + c];
  uint32_t a, b, cc;
  oov_hot(id, L.D, &a, &b, &cc);
  const double* nt = L.nt + (size_t)k * L.D * L.C + c;
  double acc = __dadd_rn(0.0, nt[(size_t)a * L.C]);
  if (b != a) acc = __dadd_rn(acc, nt[(size_t)b * L.C]);
  if (cc != b) acc = __dadd_rn(acc, nt[(size_t)cc * L.C]);
  return acc;
}

// Float32 projection row (four columns from `colc`) of slot k's vector: the table row, or for
// an out-of-vocabulary id the sum of the rows of its distinct hot positions, in a_value's
// order.  *m gets >= max_c |row| added, *terms the number of float32 addends behind the row
// (1, or up to 3): what the decision bound of the float32 keys is made of.
__device__ __forceinline__ float4 row32(const LshDev& L, int k, uint32_t id, int colc) {
  if (!(id & FS_OOV_FLAG)) return *reinterpret_cast<const float4*>(L.atab32 + ((size_t)k * L.V + id) * L.Cp + colc);
  uint32_t a, b, c;
  oov_hot(id, L.D, &a, &b, &c);
  const float* base = L.nt32 + (size_t)k * L.D * L.Cp + colc;
  float4 r = *reinterpret_cast<const float4*>(base + (size_t)a * L.Cp);
  if (b != a) {
    const float4 t = *reinterpret_cast<const float4*>(base + (size_t)b * L.Cp);
    r.x = __fadd_rn(r.x, t.x); r.y = __fadd_rn(r.y, t.y); r.z = __fadd_rn(r.z, t.z); r.w = __fadd_rn(r.w, t.w);
  }
  if (c != b) {
    const float4 t = *reinterpret_cast<const float4*>(base + (size_t)c * L.Cp);
    r.x = __fadd_rn(r.x, t.x); r.y = __fadd_rn(r.y, t.y); r.z = __fadd_rn(r.z, t.z); r.w = __fadd_rn(r.w, t.w);
  }
  return r;
}
__device__ __forceinline__ void row32_bound(const LshDev& L, int k, uint32_t id, float* m, int* terms) {
  if (!(id & FS_OOV_FLAG)) { *m += L.amax[(size_t)k * L.V + id]; *terms += 1; return; }
  uint32_t a, b, c;
  oov_hot(id, L.D, &a, &b, &c);
  const float* mx = L.ntmax + (size_t)k * L.D;
  *m += mx[a]; *terms += 1;
  if (b != a) { *m += mx[b]; *terms += 1; }
  if (c != b) { *m += mx[c]; *terms += 1; }
}

// The decision of the float32 keys, one rule for every kernel that makes it (lsh_window, k_lsh_batch,
// k_lsh_pkeys, k_lsh_scan): a column's float32 sum decides its sign iff |sum| > key_bound32, and a
// window with a column that does not is redone in float64.  am, terms: what row32_bound added up
// over the window's slots.  The relative term, terms * 2^-22 * am, is four times the worst case of
// `terms` roundings to float32 of entries whose magnitudes add up to am at most and of the float32
// additions behind them.  That holds only while an entry's rounding is relative: below 2^-126 it is
// absolute, up to 2^-150 per entry whatever its size (a float32 sum of subnormals is exact), and a
// relative bound then falls below one float32 spacing and trusts every sum that is not 0 -- hence
// the absolute term, terms * 2^-149.  (inf or NaN, from rows beyond float32: never > the bound.)
__device__ __forceinline__ float key_bound32(const LshDev& L, float am, int terms) {
  return L.bound_scale * am * ((float)terms / (float)L.n) + L.bound_abs * (float)terms;
}

__device__ __forceinline__ double q_of(const LshDev& L, uint32_t id) {
  if (!(id & FS_OOV_FLAG)) return L.q[id];
  uint32_t a, b, c;
  oov_hot(id, L.D, &a, &b, &c);
  return 1.0 + (b != a ? 1.0 : 0.0) + (c != b ? 1.0 : 0.0);
}

// g(u, v) = seqsum_d e_u[d] * e_v[d], u != v; u is a script token.  For table
// rows the sum was computed once per index (k_gtab, same order of operations).
__device__ double g_of(const LshDev& L, uint32_t u, uint32_t v) {
  const bool uo = u & FS_OOV_FLAG, vo = v & FS_OOV_FLAG;
  if (!uo && !vo) {
    if (L.gtab) {
      const int32_t r = L.sidx[u];
      if (r >= 0) return L.gtab[(size_t)r * L.V + v];
    }
    const float* eu = L.emb + (size_t)u * L.D;
    const float* ev = L.emb + (size_t)v * L.D;
    double acc = 0.0;
    for (int d = 0; d < L.D; ++d) acc = __dadd_rn(acc, __dmul_rn((double)eu[d], (double)ev[d]));
    return acc;
  }
  if (uo && vo) {
    uint32_t ua[3], va[3];
    oov_hot(u, L.D, &ua[0], &ua[1], &ua[2]);
    oov_hot(v, L.D, &va[0], &va[1], &va[2]);
    double acc = 0.0;
    for (int i = 0; i < 3; ++i) {
      if (i && ua[i] == ua[i - 1]) continue;
      bool hit = false;
      for (int j = 0; j < 3; ++j) hit = hit || va[j] == ua[i];
      if (hit) acc = __dadd_rn(acc, 1.0);
    }
    return acc;
  }
  const uint32_t row = uo ? v : u, oov = uo ? u : v;
  uint32_t h[3];
  oov_hot(oov, L.D, &h[0], &h[1], &h[2]);
  const float* e = L.emb + (size_t)row * L.D;
  double acc = 0.0;
  for (int i = 0; i < 3; ++i) {
    if (i && h[i] == h[i - 1]) continue;
    acc = __dadd_rn(acc, (double)e[h[i]]);
  }
  return acc;
}

// key h from the per-64-column ballots bal[]: bit j of the key string is column
// h*B + j, first column = most significant bit
__device__ __forceinline__ uint32_t assemble_key(const uint64_t* bal, int h, int B) {
  const int start = h * B, word = start >> 6, off = start & 63;
  uint64_t field = bal[word] >> off;
  if (off + B > 64) field |= bal[word + 1] << (64 - off);
  const uint32_t f = (uint32_t)field & ((1u << B) - 1);
  return __brev(f) >> (32 - B);
}

// (stage 1 of window_distance, behind the window's record and the comparison of the ids)
__device__ __forceinline__ bool window_distance_rest(const LshDev& L, uint32_t s, const fs_swin& sw, int same,
                                                     uint32_t diff, const uint32_t* f, const double* qf,
                                                     double ff, double rff, double* out) {
  // stage 1: the canonical sum SF slot by slot, leaving as soon as the slots still to
  // come cannot lift it to the threshold.  By Cauchy-Schwarz the remaining slots add
  // at most sqrt(SS_rem * FF_rem) (SS_rem, FF_rem = squared norms of the remaining
  // slots), so  SF_k + sqrt(SS_rem FF_rem) < (1 - thr - 1e-6) sqrt(SS) sqrt(FF)  proves
  // distance > thr + 1e-6, far outside the rounding of the canonical expression.  A
  // bucket collision between unrelated windows leaves after its first slot, which
  // costs one 32-byte record of the script window and one pair-table entry.
  const double norm = __dmul_rn(sw.rss, rff);
  if (same == L.n) {
    // identical ids in every slot: the canonical sum adds q(u_k) in slot order from 0.0,
    // which is how k_ss computed sw.ss -- the same bits, no load
    const double d = __dsub_rn(1.0, __ddiv_rn(sw.ss, norm));
    if (d != d) return false;
    *out = d;
    return true;
  }
  const double need = (1.0 - L.thr - 1e-6) * norm * (1.0 - 1e-9);
  double sf = 0.0, ssr = sw.ss, ffr = ff;
  for (int k = 0; k < L.n; ++k) {
    double g, qu, qv;
    if (qf && !(diff >> k & 1u)) {
      // the same id on both sides: g = q(u) = q(v), the fan side's (the same bits: q is a
      // function of the id)
      qu = qv = g = qf[k];
    } else {
      const uint32_t u = k ? L.stok[s + k] : sw.u0, v = f[k];
      qu = k ? q_of(L, u) : sw.qu0;
      if (u == v) g = qu;
      else if (k == 0 && sw.r0 >= 0 && !(v & FS_OOV_FLAG)) g = L.gtab[(size_t)sw.r0 * L.V + v];
      else g = g_of(L, u, v);
      qv = u == v ? qu : qf ? qf[k] : q_of(L, v);
    }
    sf = __dadd_rn(sf, g);
    if (k + 1 < L.n) {
      ssr -= qu;
      ffr -= qv;
      const double t = need - sf;
      const double rem = fmax(ssr, 0.0) * fmax(ffr, 0.0) * (1.0 + 1e-9);
      if (t > 0.0 && t * t > rem) return false;
    }
  }
  const double d = __dsub_rn(1.0, __ddiv_rn(sf, norm));
  if (d != d) return false;
  *out = d;
  return true;
}

// CosineDistance of fan window f[] to script window s (canonical), with the
// sound skips described in the file header.  Returns false when skipped or NaN.
// qf: q of the fan window's slots (LDS; lsh_neighbours_wave), or nullptr.  With it, where the
// ids were compared (stage 0), a slot that holds the same id on both sides needs no load at
// all (its q is the fan side's) and only the slots that differ fetch the script side: its id,
// q and the pair-table entry -- at n = 10 two levels of loads for the one slot instead of two
// per slot.
__device__ bool window_distance(const LshDev& L, uint32_t s, const uint32_t* f, const double* qf,
                                double ff, double rff, double* out) {
  // stage 0: integer only.  With all table norms in [sqrt(q_min), sqrt(q_max)] and
  // no OOV vector involved, m identical slots bound the cosine by
  // (m q_max + (n-m) c_max q_max) / (n q_min); m_min is the smallest m for which that
  // reaches 1 - threshold (host side, lsh_dev).
  int same = -1;
  uint32_t diff = 0xFFFFFFFFu;                  // bit k: slot k holds different ids (all: not compared)
  // (the window's record requested with its ids: one level for the two)
  fs_swin sw = L.sw[s];
  if (L.m_min > 0) {
    // (the window's ids requested together: stok is padded by a window)
    const uint4* sp = reinterpret_cast<const uint4*>(L.stok + s);
    same = 0;
    diff = 0;
    uint32_t anyoov = 0;
#pragma unroll
    for (int q4 = 0; q4 < FS_MAX_WINDOW / 4; ++q4) {
      if (4 * q4 >= L.n) break;
      const uint4 t = sp[q4];
      const uint32_t u4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * q4 + k < L.n) {
          const bool eq = u4[k] == f[4 * q4 + k];
          same += eq;
          diff |= eq ? 0u : 1u << (4 * q4 + k);
          anyoov |= u4[k] | f[4 * q4 + k];
        }
    }
    asm volatile("" : "+v"(sw.ss), "+v"(sw.rss), "+v"(sw.qu0), "+v"(sw.u0), "+v"(sw.r0));
    if (anyoov & FS_OOV_FLAG) { same = -1; diff = 0xFFFFFFFFu; }
    else if (L.m_min > 0 && same < L.m_min) return false;
  }
  return window_distance_rest(L, s, sw, same, diff, f, qf, ff, rff, out);
}

// window_distance for k_lsh_batch, the window size at compile time.  The same first level of
// loads (the window's record and ids); a window that differs from the fan window in three slots
// or fewer -- every real neighbour -- then fetches what the canonical sum needs of those slots
// together: their 16-byte {q, pair-table row, id} records (k_spos) in one level, the pair-table
// entries in the next, where window_distance goes id -> q, id -> row -> entry slot after slot.
// The same arithmetic in the same order; everything else (bucket collisions of unrelated
// windows, which leave after a slot or two; OOV ids) takes window_distance's own loop.
template <int N>
__device__ __forceinline__ bool window_distance_flat(const LshDev& L, uint32_t s, const uint32_t* f,
                                                     const double* qf, double ff, double rff, double* out) {
  const fs_swin sw = L.sw[s];
  const uint4* sp = reinterpret_cast<const uint4*>(L.stok + s);
  uint32_t u[4 * ((N + 3) / 4)];
#pragma unroll
  for (int q4 = 0; q4 < (N + 3) / 4; ++q4) {
    const uint4 t = sp[q4];
    u[4 * q4] = t.x; u[4 * q4 + 1] = t.y; u[4 * q4 + 2] = t.z; u[4 * q4 + 3] = t.w;
  }
  uint32_t diff = 0, anyoov = 0;
  int same = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const bool eq = u[k] == f[k];
    same += eq;
    diff |= eq ? 0u : 1u << k;
    anyoov |= u[k] | f[k];
  }
  if (anyoov & FS_OOV_FLAG) return window_distance_rest(L, s, sw, -1, 0xFFFFFFFFu, f, qf, ff, rff, out);
  if (L.m_min > 0 && same < L.m_min) return false;
  if (!L.spos || !L.gtab || N - same > 3)
    return window_distance_rest(L, s, sw, L.m_min > 0 ? same : -1, L.m_min > 0 ? diff : 0xFFFFFFFFu, f, qf, ff, rff, out);
  const double norm = __dmul_rn(sw.rss, rff);
  if (same == N) {
    const double d = __dsub_rn(1.0, __ddiv_rn(sw.ss, norm));
    if (d != d) return false;
    *out = d;
    return true;
  }
  // the (at most three) slots that differ
  int kd[3];
  uint32_t rest = diff;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    kd[i] = rest ? __ffs((int)rest) - 1 : -1;
    rest &= rest - 1;
  }
  uint4 rec[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (kd[i] >= 0) rec[i] = *reinterpret_cast<const uint4*>(L.spos + s + kd[i]);
  double gd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    gd[i] = 0.0;
    if (kd[i] >= 0) {
      const int32_t row = (int32_t)rec[i].z;
      gd[i] = row >= 0 ? L.gtab[(size_t)row * L.V + f[kd[i]]] : g_of(L, rec[i].w, f[kd[i]]);
    }
  }
  double sf = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double g = qf[k];
    g = k == kd[0] ? gd[0] : g; g = k == kd[1] ? gd[1] : g; g = k == kd[2] ? gd[2] : g;
    sf = __dadd_rn(sf, g);
  }
  const double d = __dsub_rn(1.0, __ddiv_rn(sf, norm));
  if (d != d) return false;
  *out = d;
  return true;
}

}  // namespace
#pragma clang diagnostic pop
