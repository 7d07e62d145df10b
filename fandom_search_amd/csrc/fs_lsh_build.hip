// fs_lsh_build.hip -- the LSH index (fs_lsh_build), built once per script on demand.
//
// Engine.store_vector for every script window: the script window keys on the device, CSR
// buckets per table in ascending window order; and everything the search kernels look up.
//   k_nt, k_nt32, k_atab      the normals transposed, the per-token projection tables A[k][v][c]
//                             and their float32 copies with the rows' largest magnitudes
//   k_embT, k_gtab            pair dot products g(script row, table row)
//   k_ss, k_spos              per script window / script token: what the canonical distance reads
//   k_keys                    keys of the script windows, a wave per window
//   k_bucket_count, _offsets, _fill, _sort, _sort_big      the CSR buckets
//   k_selflev                 (fs_launch_selflev) Levenshtein of every script window against the
//                             strings of its own ids, once per string table
//   k_comp_map                (fs_launch_comp_map) component ids of a batch's tokens
// Host side: lsh_dev (an index as the kernels see it), lsh_m_min, the wildcard-key filter and
// the one-slot maps (build_wild_filter, build_emap), the component ids of tables with
// near-synonyms (fs_build_components: union-find over the near pairs) and the share rule's
// index (fs_build_share: components of the angular relation, subset-key filter, map and lists).
#include "fs_lsh.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

using namespace fsdev;

namespace {

// ---- build kernels -----------------------------------------------------------

__global__ void k_nt(const double* __restrict__ normals, int n, int D, int C,
                     double* __restrict__ nt) {
  // nt[k][d][c] = normals[c][k*D + d]
  const size_t total = (size_t)n * D * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const size_t kd = i / C;
    nt[i] = normals[(size_t)c * n * D + kd];
  }
}

// float32 copy of nt, rows padded to Cp, and the rows' largest magnitudes (rounded up)
__global__ __launch_bounds__(256) void k_nt32(const double* __restrict__ nt, int rows, int C, int Cp,
                                              float* __restrict__ nt32, float* __restrict__ ntmax) {
  __shared__ float s_m[4];
  const int r = blockIdx.x;
  if (r >= rows) return;
  float mx = 0.0f;
  for (int c = threadIdx.x; c < Cp; c += blockDim.x) {
    const double v = c < C ? nt[(size_t)r * C + c] : 0.0;
    nt32[(size_t)r * Cp + c] = (float)v;
    mx = fmaxf(mx, __double2float_ru(fabs(v)));
  }
  for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) ntmax[r] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}

// A[k][v][c] = seqsum_d nt[k][d][c] * (double)E[v][d]; block = one (k, v)
__global__ __launch_bounds__(256) void k_atab(const double* __restrict__ nt,
                                              const float* __restrict__ emb, uint32_t V, int D,
                                              int C, int Cp, double* __restrict__ atab,
                                              float* __restrict__ atab32,
                                              float* __restrict__ amax) {
  __shared__ float s_m[4];
  const uint32_t v = blockIdx.x;
  const int k = blockIdx.y;
  const float* e = emb + (size_t)v * D;
  const double* ntk = nt + (size_t)k * D * C;
  float mx = 0.0f;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    double acc = 0.0;
    for (int d = 0; d < D; ++d)
      acc = __dadd_rn(acc, __dmul_rn(ntk[(size_t)d * C + c], (double)e[d]));
    const size_t r = (size_t)k * V + v;
    atab[r * C + c] = acc;
    atab32[r * Cp + c] = (float)acc;
    mx = fmaxf(mx, __double2float_ru(fabs(acc)));          // rounded up
  }
  for (int c = C + threadIdx.x; c < Cp; c += blockDim.x) atab32[((size_t)k * V + v) * Cp + c] = 0.0f;
  for (int d = 32; d > 0; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0)
    amax[(size_t)k * V + v] = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}

// embT[d][v] = (double) E[v][d]: coalesced reads for k_gtab
__global__ void k_embT(const float* __restrict__ emb, uint32_t V, int D, float* __restrict__ embT) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  for (int d = 0; d < D; ++d) embT[(size_t)d * V + v] = emb[(size_t)v * D + d];
}

// gtab[r][v] = seqsum_d E[srow[r]][d] * E[v][d]  (canonical: mul then add, d ascending)
__global__ __launch_bounds__(256) void k_gtab(const float* __restrict__ emb,
                                              const float* __restrict__ embT, uint32_t V, int D,
                                              const uint32_t* __restrict__ srow,
                                              double* __restrict__ gtab) {
  extern __shared__ float s_u[];     // the script row, D floats
  const uint32_t r = blockIdx.y;
  const float* eu = emb + (size_t)srow[r] * D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) s_u[d] = eu[d];
  __syncthreads();
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  double acc = 0.0;
  for (int d = 0; d < D; ++d)
    acc = __dadd_rn(acc, __dmul_rn((double)s_u[d], (double)embT[(size_t)d * V + v]));
  gtab[(size_t)r * V + v] = acc;
}

__global__ void k_ss(const uint32_t* __restrict__ stok, uint32_t W, LshDev L,
                     double* __restrict__ ss, fs_swin* __restrict__ sw) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double acc = 0.0;
  for (int k = 0; k < L.n; ++k) acc = __dadd_rn(acc, q_of(L, stok[w + k]));
  ss[w] = acc;
  fs_swin r;
  r.ss = acc;
  r.rss = __dsqrt_rn(acc);
  r.u0 = stok[w];
  r.qu0 = q_of(L, r.u0);
  r.r0 = (L.gtab && !(r.u0 & FS_OOV_FLAG)) ? L.sidx[r.u0] : -1;
  sw[w] = r;
}

// {q, pair-table row, id} of every script token: what window_distance_flat reads per slot
__global__ void k_spos(const uint32_t* __restrict__ stok, uint32_t n_script, LshDev L, fs_spos* __restrict__ spos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_script) return;
  fs_spos r;
  r.id = stok[i];
  r.q = q_of(L, r.id);
  r.row = (L.gtab && !(r.id & FS_OOV_FLAG)) ? L.sidx[r.id] : -1;
  spos[i] = r;
}

// keys of the windows of a token stream; one wave per window
__global__ __launch_bounds__(256) void k_keys(LshDev L, const uint32_t* __restrict__ tok,
                                              uint32_t n_windows, uint32_t* __restrict__ keys) {
  __shared__ uint64_t s_bal[4][32];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int NW = (L.C + 63) >> 6;
  for (uint32_t w = blockIdx.x * 4 + wave; w < n_windows; w += gridDim.x * 4) {
    for (int ch = 0; ch < NW; ++ch) {
      const int c = ch * 64 + lane;
      bool bit = false;
      if (c < L.C) {
        double acc = a_value(L, 0, tok[w], c);
        for (int k = 1; k < L.n; ++k) acc = __dadd_rn(acc, a_value(L, k, tok[w + k], c));
        bit = acc > 0.0;
      }
      const uint64_t b = __ballot(bit);
      if (lane == 0) s_bal[wave][ch] = b;
    }
    if (lane == 0) s_bal[wave][NW] = 0;
    __builtin_amdgcn_wave_barrier();
    if (lane < L.H) keys[(size_t)w * L.H + lane] = assemble_key(s_bal[wave], lane, L.B);
    __builtin_amdgcn_wave_barrier();
  }
}

// string id == vector id: Levenshtein of every script window against the strings of its
// own ids, one wave per window (FS_NONE where lev_wave reports a bad string or an
// overflow: the search then computes that match itself and reports the same)
__global__ __launch_bounds__(256) void k_selflev(GramIndexDev g, CorpusDev c, uint32_t W,
                                                 uint32_t* __restrict__ selflev) {
  __shared__ uint32_t s_la[4][FS_LEV_MAX + 2], s_lb[4][FS_LEV_MAX + 2];
  __shared__ uint32_t s_ids[4][FS_MAX_WINDOW];
  __shared__ fs_status s_st[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (uint32_t w = blockIdx.x * 4 + wave; w < W; w += gridDim.x * 4) {
    if (lane < g.n) s_ids[wave][lane] = g.stok[w + lane];
    if (lane == 0) { s_st[wave].bad_string = 0; s_st[wave].lev_overflow = 0; }
    __builtin_amdgcn_wave_barrier();
    const bool oov = lane < g.n && (s_ids[wave][lane] & FS_OOV_FLAG);
    uint32_t v = FS_NONE;
    if (!__any(oov)) {
      v = lev_wave(g, w, s_ids[wave], c.chars, c.coff, c.n_str, &s_st[wave], s_la[wave], s_lb[wave]);
      __builtin_amdgcn_wave_barrier();
      if (s_st[wave].bad_string | s_st[wave].lev_overflow) v = FS_NONE;
    }
    if (lane == 0) selflev[w] = v;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- CSR buckets on the device (Engine.store_vector for every script window) ----------
// boff[h][k+1] counts the windows with key k in table h, a scan turns the counts into
// offsets, a scatter fills bids in arrival order, and every bucket is then sorted by window
// index: the reference's buckets list their windows in insertion (= ascending) order, and
// the order decides UniqueFilter's and NearestFilter's ties.
__global__ void k_bucket_count(const uint32_t* __restrict__ keys, uint32_t W, int H, uint32_t nb,
                               uint32_t* __restrict__ boff) {
  const uint64_t total = (uint64_t)W * H;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = (uint32_t)(i % H);
    atomicAdd(&boff[(size_t)h * (nb + 1) + keys[i] + 1], 1u);
  }
}

// one workgroup per table: counts -> offsets in place (boff[h][0] = 0), and a copy of the
// bucket starts as the scatter's cursors
__global__ __launch_bounds__(256) void k_bucket_offsets(uint32_t nb, uint32_t* __restrict__ boff,
                                                        uint32_t* __restrict__ cursor) {
  __shared__ uint32_t s_w32[4];
  uint32_t* off = boff + (size_t)blockIdx.x * (nb + 1);
  uint32_t* cur = cursor + (size_t)blockIdx.x * nb;
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < nb; b0 += 256) {
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < nb ? off[b + 1] : 0u;
    uint32_t tot;
    const uint32_t excl = block_excl_scan(v, s_w32, &tot);
    if (b < nb) {
      off[b + 1] = carry + excl + v;
      cur[b] = carry + excl;
    }
    carry += tot;
    __syncthreads();
  }
}

__global__ void k_bucket_fill(const uint32_t* __restrict__ keys, uint32_t W, int H, uint32_t nb,
                              uint32_t* __restrict__ cursor, uint32_t* __restrict__ bids) {
  const uint64_t total = (uint64_t)W * H;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = (uint32_t)(i % H), w = (uint32_t)(i / H);
    const uint32_t at = atomicAdd(&cursor[(size_t)h * nb + keys[i]], 1u);
    bids[(size_t)h * W + at] = w;
  }
}

// ascending window index inside every bucket: a thread sorts a bucket of up to kSmallBucket
// entries by insertion; larger ones are listed for k_bucket_sort_big
constexpr uint32_t kSmallBucket = 48;
__global__ void k_bucket_sort(uint32_t W, int H, uint32_t nb, const uint32_t* __restrict__ boff,
                              uint32_t* __restrict__ bids, uint32_t* __restrict__ big,
                              uint32_t* __restrict__ n_big) {
  const uint64_t total = (uint64_t)nb * H;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = (uint32_t)(i / nb), b = (uint32_t)(i % nb);
    const uint32_t* off = boff + (size_t)h * (nb + 1) + b;
    const uint32_t e0 = off[0], m = off[1] - e0;
    if (m < 2) continue;
    if (m > kSmallBucket) { big[atomicAdd(n_big, 1u)] = (uint32_t)i; continue; }
    uint32_t* v = bids + (size_t)h * W + e0;
    for (uint32_t a = 1; a < m; ++a) {
      const uint32_t x = v[a];
      uint32_t c = a;
      while (c > 0 && v[c - 1] > x) { v[c] = v[c - 1]; --c; }
      v[c] = x;
    }
  }
}

// a large bucket (many script windows with one key: a repeated passage): one workgroup, every
// entry's place is the number of smaller entries (window indices are distinct)
__global__ __launch_bounds__(256) void k_bucket_sort_big(uint32_t W, uint32_t nb,
                                                         const uint32_t* __restrict__ boff,
                                                         uint32_t* __restrict__ bids,
                                                         const uint32_t* __restrict__ big,
                                                         const uint32_t* __restrict__ n_big,
                                                         uint32_t* __restrict__ tmp) {
  for (uint32_t j = blockIdx.x; j < *n_big; j += gridDim.x) {
    const uint32_t i = big[j], h = i / nb, b = i % nb;
    const uint32_t* off = boff + (size_t)h * (nb + 1) + b;
    const uint32_t e0 = off[0], m = off[1] - e0;
    uint32_t* v = bids + (size_t)h * W + e0;
    uint32_t* t = tmp + (size_t)h * W + e0;
    for (uint32_t a = threadIdx.x; a < m; a += blockDim.x) {
      const uint32_t x = v[a];
      uint32_t r = 0;
      for (uint32_t c = 0; c < m; ++c) r += v[c] < x;
      t[r] = x;
    }
    __syncthreads();
    for (uint32_t a = threadIdx.x; a < m; a += blockDim.x) v[a] = t[a];
    __syncthreads();
  }
}

__global__ void k_comp_map(const uint32_t* __restrict__ tok, uint32_t n, const uint32_t* __restrict__ comp,
                           uint32_t n_vec, uint32_t* __restrict__ out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t t = tok[i];
    out[i] = t < n_vec ? comp[t] : 0u;
  }
}

}  // namespace

// ---- host side -----------------------------------------------------------------

LshDev lsh_dev(const fs_index* ix) {
  LshDev L;
  L.atab = ix->d_atab.p; L.nt = ix->d_nt.p; L.boff = ix->d_boff.p; L.bids = ix->d_bids.p;
  L.ss = ix->d_ss.p; L.sw = ix->d_sw.p; L.q = ix->d_q.p; L.emb = ix->d_emb.p; L.stok = ix->d_stok.p;
  L.gtab = ix->d_gtab.n > 1 ? ix->d_gtab.p : nullptr; L.sidx = ix->d_sidx.p;
  L.spos = ix->d_spos.n > 1 ? ix->d_spos.p : nullptr;
  L.lsh_cnt = ix->d_lsh_cnt.n > 1 ? reinterpret_cast<unsigned long long*>(ix->d_lsh_cnt.p) : nullptr;
  L.share_cnt = nullptr; L.oovmap = nullptr; L.log2_oovmap = 0; L.compa = nullptr; L.ssig = nullptr; L.sharef = nullptr; L.smap = nullptr; L.slists = nullptr; L.log2_smap = 0; L.log2_sharef = 0; L.share_flags = 0;
  L.share_lim = 0.0f; L.share_scale = 0.0; L.share_phi = 1.0; L.share_tau = 0.0; L.share_gamma = 1.0;
  if (ix->share_flags) {
    L.compa = ix->d_compa.p; L.ssig = ix->d_ssig.p; L.sharef = ix->d_sharef.p;
    L.log2_sharef = ix->log2_sharef; L.share_flags = ix->share_flags;
    if (ix->d_share_cnt.n > 1) L.share_cnt = reinterpret_cast<unsigned long long*>(ix->d_share_cnt.p);
    if (ix->log2_oovmap) { L.oovmap = reinterpret_cast<const uint2*>(ix->d_oovmap.p); L.log2_oovmap = ix->log2_oovmap; }
    L.smap = reinterpret_cast<const uint2*>(ix->d_smap.p); L.slists = reinterpret_cast<const uint4*>(ix->d_slists.p); L.log2_smap = ix->log2_smap;
    L.share_gamma = ix->share_gamma;
    L.share_tau = 1.0 - ix->cfg.distance_threshold - 1e-6;
    L.share_phi = (1.0 - L.share_tau * L.share_tau) / (1.0 - L.share_gamma * L.share_gamma);
    L.share_lim = (float)((1.0 - L.share_phi) * (1.0 - 1e-6));
    L.share_scale = ldexp(1.0, 20) / std::max(ix->info.norm_max * ix->info.norm_max * (1.0 + 1e-9), 3.0);
  }
  L.emap = nullptr; L.log2_emap = 0; L.emap_comp = 0; L.skeys = ix->d_skeys.n > 1 ? ix->d_skeys.p : nullptr;
  L.atab32 = ix->d_atab32.n > 1 ? ix->d_atab32.p : nullptr; L.amax = ix->d_amax.p;
  L.nt32 = ix->d_nt32.p; L.ntmax = ix->d_ntmax.p;
  L.wild = nullptr; L.log2_wild = 0; L.wild_tok = nullptr; L.selflev = nullptr; L.wmap = nullptr; L.log2_wmap = 0;
  L.V = (uint32_t)ix->n_vec; L.W = (uint32_t)ix->n_windows;
  L.n = (int)ix->cfg.window_size; L.H = (int)ix->cfg.number_of_hashes;
  L.B = (int)ix->cfg.hash_dimensions; L.D = (int)ix->cfg.emb_dim; L.C = L.H * L.B;
  L.Cp = (L.C + 3) & ~3;
  L.nn = (int)ix->cfg.nearest_n; L.unique = ix->cfg.unique_filter ? 1 : 0;
  L.thr = ix->cfg.distance_threshold;
  L.cmax = ix->lsh_cmax;
  {
    // n * 2^-22; FS_LSH_F32_SLACK multiplies it (tests force the float64 fallback),
    // FS_LSH_F32=0 disables the float32 path
    L.bound_scale = (float)((double)ix->cfg.window_size * ldexp(1.0, -22) * ix->sw.lsh_f32_slack);
    L.bound_abs = (float)(ldexp(1.0, -149) * ix->sw.lsh_f32_slack);
    if (!ix->sw.lsh_f32) L.atab32 = nullptr;
    L.m_min = ix->lsh_m_min;
    L.diag = ix->sw.lsh_diag;
    L.serial_neighbours = ix->sw.lsh_serial ? 1 : 0;
  }
  return L;
}

// smallest number of id-identical slots with which a window pair can reach
// cos >= 1 - thr - 1e-6 (n: only identical windows)
static int lsh_m_min(const fs_index* ix) {
  const int n = (int)ix->cfg.window_size;
  const double qmin = ix->info.norm_min * ix->info.norm_min, qmax = ix->info.norm_max * ix->info.norm_max;
  if (!(qmin > 0.0) || !(ix->lsh_cmax < 1.0)) return 0;
  const double lim = (1.0 - ix->cfg.distance_threshold - 1e-6) * n * qmin * (1.0 - 1e-9);
  int m = 0;
  while (m <= n && (m + (n - m) * ix->lsh_cmax) * qmax < lim) ++m;
  return m > n ? n : m;          // n + 1 would mean "nothing can match": exact windows still do
}

// The grouped filter of one-slot-wildcard keys (fs_hash.h) over the id sequence `st` (vector ids,
// or component ids): log2 of its 16-byte blocks and the blocks, about 24 filter bits per key.
static int build_wild_filter(const std::vector<uint32_t>& st, uint64_t W, int n, std::vector<uint32_t>* out) {
  int lb = 8;
  while (lb < 26 && ((uint64_t)128 << lb) < W * n * 24) ++lb;
  out->assign((size_t)4 << lb, 0u);
  for (uint64_t w = 0; w < W; ++w) {
    uint32_t term[FS_MAX_WINDOW], fold = 0, gfold[3] = {0, 0, 0};
    for (int k = 0; k < n; ++k) {
      term[k] = fs_rotl(fs_premix(st[w + k]), fs_rot_of(n - 1 - k));
      fold ^= term[k];
      gfold[fs_wild_group(k, n)] ^= term[k];
    }
    for (int k = 0; k < n; ++k) {
      const uint32_t h = fs_wild_fkey(fold, term[k], k);
      const int X = fs_wild_group(k, n);
      uint32_t* blk = out->data() + 4 * (size_t)fs_wild_block(fold ^ gfold[X], X, lb);
      for (int i = 0; i < 4; ++i) blk[i] |= 1u << fs_wild_fbit(h, i);
    }
  }
  return lb;
}

// The one-slot-wildcard keys of every distinct script n-gram (by vector ids: gram g's first
// window is gpos[g][0]) as an exact map key -> g, the keys made of `ids` (the script's vector
// ids, or their component ids): buckets of four {key, g + 1}, a full bucket spills into the next
// (k_lsh_batch gives a window up to the bucket walk when it meets a full one).
static int build_emap(fs_index* ix, const std::vector<uint32_t>& ids, DBuf<uint32_t>* out, int* log2_out) {
  const int n = (int)ix->cfg.window_size;
  const uint32_t nn = ix->cfg.nearest_n;
  const uint32_t G = ix->n_grams;
  *log2_out = 0;
  if (!G || !ix->d_gpos.p) return FS_OK;
  std::vector<uint32_t> gpos((size_t)G * nn);
  FS_HIP(hipMemcpy(gpos.data(), ix->d_gpos.p, gpos.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  int lm = 8;                                    // two buckets per entry: a full one (four entries) is rare
  while (lm < 26 && ((uint64_t)1 << lm) < 2 * (uint64_t)G * n) ++lm;
  std::vector<uint32_t> emap((size_t)8 << lm, 0u);
  const uint32_t mask = (1u << lm) - 1;
  for (uint32_t g = 0; g < G; ++g) {
    const uint32_t w = gpos[(size_t)g * nn];
    uint32_t term[FS_MAX_WINDOW], fold = 0;
    for (int k = 0; k < n; ++k) {
      term[k] = fs_rotl(fs_premix(ids[w + k]), fs_rot_of(n - 1 - k));
      fold ^= term[k];
    }
    for (int k = 0; k < n; ++k) {
      const uint32_t h = fs_wild_key(fold, term[k], k);
      uint32_t bkt = fs_wmap_slot(h, lm);
      for (;;) {
        uint32_t* e = emap.data() + 8 * (size_t)bkt;
        int at = 0;
        while (at < 4 && e[2 * at + 1]) ++at;
        if (at < 4) { e[2 * at] = h; e[2 * at + 1] = g + 1; break; }
        bkt = (bkt + 1) & mask;
      }
    }
  }
  FS_TRY(out->upload(emap.data(), emap.size(), ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  *log2_out = lm;
  return FS_OK;
}

// Tables with near-synonyms (every real embedding table): the proof that a neighbour within the
// threshold shares n or n - 1 vector ids with the window fails, but a weaker one holds.  With
// x_k = |f_k|, y_k = |s_k|, c_k = cos(f_k, s_k):
//   cos(F, S) |x| |y| = sum x_k y_k c_k = sum x_k y_k - sum d_k <= |x| |y| - sum d_k,
//   d_k = (1 - c_k) x_k y_k >= 0,
// so a record (cos > 1 - thr) needs sum d_k < thr |x| |y| <= T = thr n a_max^2, and at most ONE
// slot has d_k >= T / 2, i.e. cos(f_k, s_k) <= 1 - T / (2 |f_k| |s_k|).  Call a pair of a script
// vector and a table vector above that line *near* (unit vectors, n = 6, thr = 0.1: cos > 0.7)
// and give every table vector the id of its connected component in the graph of near pairs:
// a window can have a neighbour within the threshold only if its component ids equal a
// script window's in n - 1 slots or more.  That is the test the filters of the
// one-slot case make on vector ids (k_scan_near, the wildcard keys), here made on component
// ids; the windows that pass get the full LSH work (their per-n-gram record where their vector
// ids are a script n-gram's).  Sound: a filter only removes windows that cannot have a
// neighbour.  Not used when the components are too coarse to filter (one of them holding an
// eighth of the table or more: zero rows, hubs of tiny norm) or a side holds OOV vectors.
static int fs_build_components(fs_index* ix) {
  ix->syn_ok = false;
  const int n = (int)ix->cfg.window_size, D = (int)ix->cfg.emb_dim;
  const uint64_t V = ix->n_vec, W = ix->n_windows;
  if (!ix->sw.lsh_syn || ix->script_oov || !W || V > FS_MAX_EXACT_ID || n < 6 ||
      !(n <= 10 || n == 12) || !(ix->info.norm_max > 0.0)) return FS_OK;
  std::vector<uint32_t> st(ix->n_script);
  FS_HIP(hipMemcpyAsync(st.data(), ix->d_stok.p, ix->n_script * sizeof(uint32_t), hipMemcpyDeviceToHost, ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  std::vector<uint32_t> rows_u;
  {
    std::vector<uint8_t> seen(V, 0);
    for (uint32_t id : st)
      if (!seen[id]) { seen[id] = 1; rows_u.push_back(id); }
  }
  // near pairs (script vector, table vector) from the device
  const uint32_t cap = 1u << 23;
  DBuf<float> embT;
  DBuf<uint32_t> d_rows_u, d_cnt;
  DBuf<uint2> d_pairs;
  FS_TRY(embT.reserve((size_t)V * D));
  FS_TRY(d_rows_u.upload(rows_u.data(), rows_u.size(), ix->stream));
  FS_TRY(d_cnt.reserve(1));
  FS_TRY(d_pairs.reserve(cap));
  FS_HIP(hipMemsetAsync(d_cnt.p, 0, sizeof(uint32_t), ix->stream));
  const double T = ix->cfg.distance_threshold * n * ix->info.norm_max * ix->info.norm_max * (1.0 + 1e-6);
  FS_TRY(fs_launch_near_pairs(ix->d_emb.p, V, D, d_rows_u.p, (uint32_t)rows_u.size(), ix->d_q.p, embT.p,
                              (float)(T / 2.0), -2.0f, d_pairs.p, cap, d_cnt.p, ix->stream));
  uint32_t n_pairs = 0;
  FS_HIP(hipMemcpyAsync(&n_pairs, d_cnt.p, sizeof n_pairs, hipMemcpyDeviceToHost, ix->stream));
  FS_HIP(hipStreamSynchronize(ix->stream));
  if (n_pairs > cap) return FS_OK;                 // (far too many near pairs: nothing to filter with)
  std::vector<uint2> pairs(n_pairs);
  if (n_pairs) FS_HIP(hipMemcpy(pairs.data(), d_pairs.p, (size_t)n_pairs * sizeof(uint2), hipMemcpyDeviceToHost));
  // connected components (union-find), ids dense in order of the smallest member
  std::vector<uint32_t> parent(V);
  for (uint64_t v = 0; v < V; ++v) parent[v] = (uint32_t)v;
  auto find = [&](uint32_t v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
  };
  for (const uint2& e : pairs) {
    const uint32_t a = find(e.x), b = find(e.y);
    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
  }
  std::vector<uint32_t> comp(V), size;
  {
    std::vector<uint32_t> id_of(V, FS_NONE);
    for (uint64_t v = 0; v < V; ++v) {
      const uint32_t r = find((uint32_t)v);
      if (id_of[r] == FS_NONE) { id_of[r] = (uint32_t)size.size(); size.push_back(0); }
      comp[v] = id_of[r];
      ++size[comp[v]];
    }
  }
  ix->n_comp = (uint32_t)size.size();
  ix->comp_sizes = size;
  ix->comp_largest = *std::max_element(size.begin(), size.end());
  if ((uint64_t)ix->comp_largest * 8 > V && ix->comp_largest > 64) return FS_OK;
  FS_TRY(ix->d_comp.upload(comp.data(), comp.size(), ix->stream));
  // the two filters of the one-slot case, over the script's component ids
  std::vector<uint32_t> sc(st.size());
  for (size_t i = 0; i < st.size(); ++i) sc[i] = comp[st[i]];
  std::vector<uint32_t> sub(1u << fs_scan_near_log2(ix), 0u);
  const int K = fs_scan_near_k(n);
  for (uint64_t i = 0; i + K <= sc.size(); ++i) {
    uint32_t word, bit;
    fs_scan_near_bit(ix, sc.data() + i, &word, &bit);
    sub[word] |= 1u << bit;
  }
  FS_TRY(ix->d_sfilter3c.upload(sub.data(), sub.size(), ix->stream));
  std::vector<uint32_t> wild;
  const int lwild = build_wild_filter(sc, W, n, &wild);
  FS_TRY(ix->d_wildc.upload(wild.data(), wild.size(), ix->stream));
  ix->log2_wildc = lwild;
  FS_TRY(build_emap(ix, sc, &ix->d_emapc, &ix->log2_emapc));
  if (n == 6) {
    // the keys of slots 2 and 3 in a filter of their own for k_scan_near (fs_scan.hip)
    std::vector<uint32_t> keys((size_t)1 << FS_NEAR6_LOG2_WORDS, 0u);
    for (uint64_t w = 0; w < W; ++w) {
      uint32_t term[6], fold = 0;
      for (int k = 0; k < 6; ++k) {
        term[k] = fs_rotl(fs_premix(sc[w + k]), fs_rot_of(5 - k));
        fold ^= term[k];
      }
      for (int k = 2; k <= 3; ++k) {
        const uint32_t h = fs_wild_key(fold, term[k], k);
        keys[fs_bloom_word(h, FS_NEAR6_LOG2_WORDS)] |= fs_bloom_mask(h);
      }
    }
    FS_TRY(ix->d_keys6c.upload(keys.data(), keys.size(), ix->stream));
  }
  FS_HIP(hipStreamSynchronize(ix->stream));
  ix->syn_ok = true;
  return FS_OK;
}

// The share rule's index side (fs_lsh_share.hip, "the share rule"): the components of the angular
// relation cos > gamma over (script vector, table vector) pairs, the proof that out-of-vocabulary
// fan tokens are far from every script vector, and the filter of the script windows' subset keys.
static int fs_build_share(fs_index* ix) {
  ix->share_flags = 0;
  const int n = (int)ix->cfg.window_size, D = (int)ix->cfg.emb_dim;
  const uint64_t V = ix->n_vec, W = ix->n_windows;
  const double gamma = ix->sw.share_gamma;
  const double tau = 1.0 - ix->cfg.distance_threshold - 1e-6;
  if (!(ix->sw.lsh_share & 3) || !W || !V || V > FS_MAX_EXACT_ID || n < 2 ||
      !(ix->info.norm_max > 0.0) || !(gamma >= 0.05 && gamma <= 0.995) || !(tau > gamma + 1e-3))
    return FS_OK;
  // (a script with out-of-vocabulary tokens: share_comp's case analysis needs 2/3 to be far)
  if (ix->script_oov && !(gamma >= 0.668)) return FS_OK;
  hipStream_t s = ix->stream;
  std::vector<uint32_t> st(ix->n_script);
  FS_HIP(hipMemcpyAsync(st.data(), ix->d_stok.p, ix->n_script * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  std::vector<uint32_t> rows_u;
  {
    std::vector<uint8_t> seen(V, 0);
    for (uint32_t id : st)
      if (!(id & FS_OOV_FLAG) && !seen[id]) { seen[id] = 1; rows_u.push_back(id); }
  }
  const uint32_t cap = 1u << 23;
  DBuf<float> embT;
  DBuf<uint32_t> d_rows_u, d_cnt;
  DBuf<uint2> d_pairs;
  FS_TRY(embT.reserve((size_t)V * D));
  FS_TRY(d_rows_u.upload(rows_u.data(), rows_u.size(), s));
  FS_TRY(d_cnt.reserve(2));
  FS_TRY(d_pairs.reserve(cap));
  FS_HIP(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(uint32_t), s));
  FS_TRY(fs_launch_near_pairs(ix->d_emb.p, V, D, d_rows_u.p, (uint32_t)rows_u.size(), ix->d_q.p, embT.p, 0.0f,
                              (float)gamma, d_pairs.p, cap, d_cnt.p, s));
  // (out-of-vocabulary fan tokens against the script's rows; with out-of-vocabulary tokens in the
  // script also those against every row a fan token may be)
  if (ix->script_oov)
    FS_TRY(fs_launch_coordmax(ix->d_emb.p, D, nullptr, (uint32_t)V, ix->d_q.p, reinterpret_cast<int*>(d_cnt.p + 1), s));
  else
    FS_TRY(fs_launch_coordmax(ix->d_emb.p, D, d_rows_u.p, (uint32_t)rows_u.size(), ix->d_q.p,
                              reinterpret_cast<int*>(d_cnt.p + 1), s));
  uint32_t res[2] = {0, 0};
  FS_HIP(hipMemcpyAsync(res, d_cnt.p, sizeof res, hipMemcpyDeviceToHost, s));
  FS_HIP(hipStreamSynchronize(s));
  const uint32_t n_pairs = res[0];
  if (n_pairs > cap) return FS_OK;                 // (far too many near pairs: nothing to filter with)
  float kappa;
  memcpy(&kappa, &res[1], sizeof kappa);
  const bool oov_far = sqrt(3.0) * (double)kappa * (1.0 + 1e-6) <= gamma - 1e-4;
  std::vector<uint2> pairs(n_pairs);
  if (n_pairs) FS_HIP(hipMemcpy(pairs.data(), d_pairs.p, (size_t)n_pairs * sizeof(uint2), hipMemcpyDeviceToHost));
  std::vector<uint32_t> parent(V);
  for (uint64_t v = 0; v < V; ++v) parent[v] = (uint32_t)v;
  auto find = [&](uint32_t v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
  };
  for (const uint2& e : pairs) {
    const uint32_t a = find(e.x), b = find(e.y);
    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
  }
  std::vector<uint32_t> comp(V), size;
  {
    std::vector<uint32_t> id_of(V, FS_NONE);
    for (uint64_t v = 0; v < V; ++v) {
      const uint32_t r = find((uint32_t)v);
      if (id_of[r] == FS_NONE) { id_of[r] = (uint32_t)size.size(); size.push_back(0); }
      comp[v] = id_of[r];
      ++size[comp[v]];
    }
  }
  ix->comp_sizes = size;                            // (fs_index_component_sizes: the angular relation's, where the rule is built)
  ix->share_comps = (uint32_t)size.size();
  ix->share_largest = *std::max_element(size.begin(), size.end());
  int flags = ix->sw.lsh_share & 47;
  if (!oov_far) {
    if (ix->script_oov) return FS_OK;               // (the script's 3-hot vectors may be near table rows: no rule)
    flags |= 8;
  }
  if ((flags & 8) || ix->script_oov) flags &= ~4;  // (a slot that agrees with anything has no share on the script's side)
  if (n > FS_MAX_WINDOW || n > 12) flags &= ~1;
  if (n > 6) flags &= ~4;                          // (run by run: the fan window's side only)
  uint64_t n_masks_all = 0;                        // subsets per script window, over its runs (fs_share_blocks)
  for (int r = 0; r < fs_share_blocks(n); ++r)
    n_masks_all += ((uint64_t)1 << (fs_share_block_start(n, r + 1) - fs_share_block_start(n, r))) - 1;
  if ((flags & 35) != 35 || W * n_masks_all > ((uint64_t)1 << 25)) flags &= ~32;   // (the enumeration needs the gate and the pairs' test)
  if (flags & 32) flags &= ~4;                     // (... and every subset of every script window in the filter)
  if (!(flags & 3)) return FS_OK;
  FS_TRY(ix->d_compa.upload(comp.data(), comp.size(), s));
  // the script's out-of-vocabulary vectors (share_comp): a component per distinct set of three
  // positions, in a map for the fan tokens; a component of its own per vector of fewer positions,
  // its pair of positions in the map so that a fan token that contains it counts as agreeing with
  // anything
  ix->log2_oovmap = 0;
  std::vector<uint32_t> oov_comp_of;               // per script token (OOV ones), by index into st
  std::vector<std::pair<uint32_t, uint32_t>> oov_entries;   // {key, component}
  auto hot_of = [&](uint32_t id, uint32_t h[3]) {
    const uint32_t code = id & ~FS_OOV_FLAG, Du = (uint32_t)D;
    h[2] = code % Du; h[1] = (code / Du) % Du; h[0] = code / (Du * Du);
    std::sort(h, h + 3);
  };
  auto q_host = [&](uint32_t id, const std::vector<double>& qv) {
    if (!(id & FS_OOV_FLAG)) return qv[id];
    uint32_t h[3];
    hot_of(id, h);
    return 1.0 + (h[1] != h[0] ? 1.0 : 0.0) + (h[2] != h[1] ? 1.0 : 0.0);
  };
  std::vector<uint32_t> sc(st.size() + FS_MAX_WINDOW, FS_NONE);
  {
    uint32_t next = (uint32_t)V;
    std::vector<std::pair<uint64_t, uint32_t>> sets;         // distinct position sets -> component
    for (size_t i = 0; i < st.size(); ++i) {
      if (!(st[i] & FS_OOV_FLAG)) { sc[i] = comp[st[i]]; continue; }
      uint32_t h[3];
      hot_of(st[i], h);
      const uint64_t set = ((uint64_t)h[0] << 40) | ((uint64_t)h[1] << 20) | h[2];
      uint32_t c = FS_NONE;
      for (const auto& e : sets)
        if (e.first == set) { c = e.second; break; }
      if (c == FS_NONE) {
        c = next++;
        sets.push_back({set, c});
        const uint32_t Du = (uint32_t)D;
        if (h[0] != h[1] && h[1] != h[2]) oov_entries.push_back({(h[0] * Du + h[1]) * Du + h[2], c});
        else if (h[0] != h[2]) oov_entries.push_back({0x80000000u | (h[0] * Du + h[2]), FS_WILD});   // two positions
      }
      sc[i] = c;
    }
    if ((uint64_t)D * D * D >= (1ull << 31)) { if (!oov_entries.empty()) return FS_OK; }
    if (!oov_entries.empty()) {
      int lo = 4;
      while (((size_t)1 << lo) < 2 * oov_entries.size()) ++lo;
      std::vector<uint32_t> m((size_t)2 << lo, 0u);
      const uint32_t mask = (1u << lo) - 1;
      for (const auto& e : oov_entries) {
        uint32_t at = fs_mix24(e.first) & mask;
        while (m[2 * at + 1]) at = (at + 1) & mask;
        m[2 * at] = e.first;
        m[2 * at + 1] = e.second + 1;                // (0: empty; FS_WILD + 1 = FS_NONE: share_comp reads it as "there")
      }
      FS_TRY(ix->d_oovmap.upload(m.data(), m.size(), s));
      ix->log2_oovmap = lo;
    }
  }
  std::vector<uint64_t> sig(W, 0);
  {
    const int b = fs_share_sig_bits(n);
    for (uint64_t w = 0; w < W; ++w)
      for (int k = 0; k < n; ++k) sig[w] |= (uint64_t)fs_share_sig(sc[w + k], n) << (k * b);
    FS_TRY(ix->d_ssig.upload(sig.data(), sig.size(), s));
  }
  if (flags & 1) {
    std::vector<double> q(V);
    FS_HIP(hipMemcpyAsync(q.data(), ix->d_q.p, V * sizeof(double), hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    const uint64_t keys = W * n_masks_all / ((flags & 4) ? 3 : 1);
    int lw = 10;
    while (lw < 26 && ((uint64_t)1 << lw) * 4 < keys * 3) ++lw;    // about 24 filter bits per key and more
    std::vector<uint32_t> f((size_t)1 << lw, 0u);
    const double phi = (1.0 - tau * tau) / (1.0 - gamma * gamma);
    for (uint64_t w = 0; w < W; ++w) {
      uint32_t t[FS_MAX_WINDOW];
      double qs[FS_MAX_WINDOW], all = 0.0;
      for (int k = 0; k < n; ++k) {
        t[k] = fs_share_term(sc[w + k], k);
        qs[k] = q_host(st[w + k], q);
        all += qs[k];
      }
      const double need = (1.0 - phi) * all * (1.0 - 1e-6);
      for (int r = 0; r < fs_share_blocks(n); ++r) {
        const int k0 = fs_share_block_start(n, r), k1 = fs_share_block_start(n, r + 1);
        for (uint32_t sub = 1; sub < (1u << (k1 - k0)); ++sub) {
          const uint32_t m = sub << k0;
          uint32_t fold = 0;
          double sum = 0.0;
          for (int k = k0; k < k1; ++k)
            if ((m >> k) & 1u) { fold ^= t[k]; sum += qs[k]; }
          if ((flags & 4) && sum < need) continue;   // (only the subsets that hold the share on this side too)
          const uint32_t h = fs_share_key(fold, m);
          f[fs_bloom_word(h, lw)] |= fs_bloom_mask(h);
        }
      }
    }
    FS_TRY(ix->d_sharef.upload(f.data(), f.size(), s));
    ix->log2_sharef = lw;
    if (flags & 32) {
      // the same keys as an exact map: key -> its script windows
      std::vector<uint64_t> ent;
      ent.reserve(W * n_masks_all);
      for (uint64_t w = 0; w < W; ++w) {
        uint32_t t[FS_MAX_WINDOW];
        for (int k = 0; k < n; ++k) t[k] = fs_share_term(sc[w + k], k);
        for (int r = 0; r < fs_share_blocks(n); ++r) {
          const int k0 = fs_share_block_start(n, r), k1 = fs_share_block_start(n, r + 1);
          for (uint32_t sub = 1; sub < (1u << (k1 - k0)); ++sub) {
            const uint32_t m = sub << k0;
            uint32_t fold = 0;
            for (int k = k0; k < k1; ++k)
              if ((m >> k) & 1u) fold ^= t[k];
            ent.push_back((uint64_t)fs_share_key(fold, m) << 32 | w);
          }
        }
      }
      std::sort(ent.begin(), ent.end());
      uint64_t distinct = 0;
      for (size_t i = 0; i < ent.size(); ++i) distinct += i == 0 || (ent[i] >> 32) != (ent[i - 1] >> 32);
      int lm = 8;                                  // two buckets per key: a full one (four entries) is rare
      while (lm < 26 && ((uint64_t)1 << lm) < 2 * distinct) ++lm;
      std::vector<uint32_t> smap((size_t)8 << lm, 0u);
      std::vector<uint4> lists;
      lists.reserve(ent.size() + distinct + 1);
      lists.push_back(make_uint4(0, 0, 0, 0));      // (a list is named by the index of its first script window: never 0)
      const uint32_t bmask = (1u << lm) - 1;
      for (size_t i = 0; i < ent.size();) {
        const uint32_t h = (uint32_t)(ent[i] >> 32);
        size_t e1 = i;
        while (e1 < ent.size() && (uint32_t)(ent[e1] >> 32) == h) ++e1;
        lists.push_back(make_uint4((uint32_t)(e1 - i), 0, 0, 0));       // its length, then its script windows
        const uint32_t first = (uint32_t)lists.size();
        for (size_t x = i; x < e1; ++x) {
          const uint32_t w = (uint32_t)ent[x];
          lists.push_back(make_uint4(w, (uint32_t)sig[w], (uint32_t)(sig[w] >> 32), 0));
        }
        uint32_t bkt = fs_wmap_slot(h, lm);
        for (;;) {
          uint32_t* e = smap.data() + 8 * (size_t)bkt;
          int at = 0;
          while (at < 4 && e[2 * at + 1]) ++at;
          if (at < 4) { e[2 * at] = h; e[2 * at + 1] = first; break; }
          bkt = (bkt + 1) & bmask;
        }
        i = e1;
      }
      FS_TRY(ix->d_smap.upload(smap.data(), smap.size(), s));
      FS_TRY(ix->d_slists.upload(reinterpret_cast<const uint32_t*>(lists.data()), lists.size() * 4, s));
      ix->log2_smap = lm;
    }
  }
  if (ix->sw.share_count) {
    FS_TRY(ix->d_share_cnt.reserve(16));
    FS_HIP(hipMemsetAsync(ix->d_share_cnt.p, 0, 16 * sizeof(uint32_t), s));
  }
  FS_HIP(hipStreamSynchronize(s));
  ix->share_gamma = gamma;
  ix->share_flags = flags | 16;                    // (bit 4: in use, whatever else is set)
  return FS_OK;
}

int fs_lsh_build(fs_index* ix) {
  if (ix->lsh_ready) return FS_OK;
  ix->lsh_m_min = lsh_m_min(ix);
  ix->near8 = fs_scan_near8_wanted(ix);
  if ((int)ix->cfg.window_size - ix->lsh_m_min == 1 && !ix->script_oov && ix->cfg.window_size >= 4 &&
      ix->n_vec <= FS_MAX_EXACT_ID) {
    // a neighbour differs from the window in at most one slot: one bit per script 3-gram
    // for the integer prefilter (k_scan_near, fs_scan.hip)
    std::vector<uint32_t> st(ix->n_script);
    FS_HIP(hipMemcpyAsync(st.data(), ix->d_stok.p, ix->n_script * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          ix->stream));
    FS_HIP(hipStreamSynchronize(ix->stream));
    std::vector<uint32_t> sub(1u << fs_scan_near_log2(ix), 0u);
    for (uint64_t i = 0; i + 3 <= ix->n_script; ++i) {
      uint32_t word, bit;
      fs_scan_near_bit(ix, st.data() + i, &word, &bit);
      sub[word] |= 1u << bit;
    }
    FS_TRY(ix->d_sfilter3.upload(sub.data(), sub.size(), ix->stream));
    // ... and the n one-slot-wildcard keys of every script window, about 24 filter bits
    // per key (k_lsh_verify drops a window none of whose keys is present)
    const int n = (int)ix->cfg.window_size;
    const uint64_t W = ix->n_windows;
    std::vector<uint32_t> wild;
    const int lwild = build_wild_filter(st, W, n, &wild);
    FS_TRY(ix->d_wild.upload(wild.data(), wild.size(), ix->stream));
    ix->log2_wild = lwild;
    // ... and as an exact map, one entry per distinct n-gram (its first window) and slot
    {
      std::vector<uint32_t> first;                       // first window of every distinct n-gram
      {
        std::vector<uint32_t> order(W);
        for (uint64_t w = 0; w < W; ++w) order[w] = (uint32_t)w;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
          return std::lexicographical_compare(st.begin() + a, st.begin() + a + n, st.begin() + b, st.begin() + b + n);
        });
        for (uint64_t i = 0; i < W; ++i)
          if (i == 0 || !std::equal(st.begin() + order[i], st.begin() + order[i] + n, st.begin() + order[i - 1]))
            first.push_back(order[i]);
      }
      // buckets of four {key, window + 1}, about one entry per bucket; a full bucket spills
      // into the next one (the kernel gives a window up when it meets a full bucket)
      int lm = 8;
      while (lm < 26 && ((uint64_t)1 << lm) < first.size() * (uint64_t)n) ++lm;
      std::vector<uint32_t> wmap((size_t)8 << lm, 0u);
      const uint32_t mask = (1u << lm) - 1;
      for (uint32_t w : first) {
        uint32_t term[FS_MAX_WINDOW], fold = 0;
        for (int k = 0; k < n; ++k) {
          term[k] = fs_rotl(fs_premix(st[w + k]), fs_rot_of(n - 1 - k));
          fold ^= term[k];
        }
        for (int k = 0; k < n; ++k) {
          const uint32_t h = fs_wild_key(fold, term[k], k);
          uint32_t bkt = fs_wmap_slot(h, lm);
          for (;;) {
            uint32_t* e = wmap.data() + 8 * (size_t)bkt;
            int at = 0;
            while (at < 4 && e[2 * at + 1]) ++at;
            if (at < 4) { e[2 * at] = h; e[2 * at + 1] = w + 1; break; }
            bkt = (bkt + 1) & mask;
          }
        }
      }
      FS_TRY(ix->d_wmap.upload(wmap.data(), wmap.size(), ix->stream));
      ix->log2_wmap = lm;
    }
    FS_TRY(build_emap(ix, st, &ix->d_emap, &ix->log2_emap));
    FS_HIP(hipStreamSynchronize(ix->stream));
  }
  if ((int)ix->cfg.window_size - ix->lsh_m_min > 1) FS_TRY(fs_build_components(ix));
  // (where neither integer prefilter applies the search is k_lsh_scan: the share rule is for it)
  if (((int)ix->cfg.window_size - ix->lsh_m_min > 1 || ix->script_oov || ix->cfg.window_size < 4 ||
       ix->n_vec > FS_MAX_EXACT_ID) && !ix->syn_ok)
    FS_TRY(fs_build_share(ix));
  if (!ix->d_normals.p) { fs_set_error("normals are required for the LSH pipeline"); return FS_E_INVALID; }
  hipStream_t s = ix->stream;
  const int n = (int)ix->cfg.window_size, D = (int)ix->cfg.emb_dim;
  const int H = (int)ix->cfg.number_of_hashes, B = (int)ix->cfg.hash_dimensions, C = H * B;
  const uint64_t V = ix->n_vec, W = ix->n_windows;
  FS_TRY(ix->d_nt.reserve((size_t)n * D * C));
  FS_TRY(ix->d_atab.reserve((size_t)n * V * C));
  const int Cp = (C + 3) & ~3;
  FS_TRY(ix->d_atab32.reserve((size_t)n * V * Cp + 4));
  FS_TRY(ix->d_amax.reserve((size_t)n * V + 1));
  FS_TRY(ix->d_ss.reserve(W));
  FS_TRY(ix->d_sw.reserve(W));
  hipLaunchKernelGGL(k_nt, dim3(1024), dim3(256), 0, s, ix->d_normals.p, n, D, C, ix->d_nt.p);
  FS_TRY(ix->d_nt32.reserve((size_t)n * D * Cp + 4));
  FS_TRY(ix->d_ntmax.reserve((size_t)n * D + 1));
  hipLaunchKernelGGL(k_nt32, dim3((uint32_t)(n * D)), dim3(256), 0, s, ix->d_nt.p, n * D, C, Cp, ix->d_nt32.p, ix->d_ntmax.p);
  if (V)
    hipLaunchKernelGGL(k_atab, dim3((uint32_t)V, n), dim3(256), 0, s, ix->d_nt.p, ix->d_emb.p,
                       (uint32_t)V, D, C, Cp, ix->d_atab.p, ix->d_atab32.p, ix->d_amax.p);
  FS_HIP(hipGetLastError());
  // pair dot products g(script row, table row): one 8-byte lookup per window slot
  // instead of D multiply-adds when a candidate's exact distance is needed.  Capped
  // at 64 GiB of the 288 GB HBM; beyond that g is computed on the fly.
  {
    std::vector<uint32_t> stok_h(ix->n_script);
    FS_HIP(hipMemcpyAsync(stok_h.data(), ix->d_stok.p, ix->n_script * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> sidx(std::max<uint64_t>(V, 1), -1);
    std::vector<uint32_t> srow;
    for (uint32_t id : stok_h)
      if (!(id & FS_OOV_FLAG) && sidx[id] < 0) { sidx[id] = (int32_t)srow.size(); srow.push_back(id); }
    FS_TRY(ix->d_sidx.upload(sidx.data(), sidx.size(), s));
    const uint64_t bytes = (uint64_t)srow.size() * V * sizeof(double);
    if (!srow.empty() && V && bytes <= (64ull << 30) && !ix->sw.lsh_no_gtab) {
      DBuf<uint32_t> d_srow;
      DBuf<float> embT;
      FS_TRY(d_srow.upload(srow.data(), srow.size(), s));
      FS_TRY(embT.reserve((size_t)V * D));
      FS_TRY(ix->d_gtab.reserve((size_t)srow.size() * V));
      hipLaunchKernelGGL(k_embT, dim3((uint32_t)((V + 255) / 256)), dim3(256), 0, s, ix->d_emb.p,
                         (uint32_t)V, D, embT.p);
      for (size_t r0 = 0; r0 < srow.size(); r0 += 32768) {        // grid.y limit
        const uint32_t rows = (uint32_t)std::min<size_t>(32768, srow.size() - r0);
        hipLaunchKernelGGL(k_gtab, dim3((uint32_t)((V + 255) / 256), rows), dim3(256),
                           D * sizeof(float), s, ix->d_emb.p, embT.p, (uint32_t)V, D,
                           d_srow.p + r0, ix->d_gtab.p + r0 * V);
      }
      FS_HIP(hipGetLastError());
      FS_HIP(hipStreamSynchronize(s));
    }
  }
  const uint32_t nb = 1u << B;
  FS_TRY(ix->d_boff.reserve((size_t)H * (nb + 1)));
  FS_TRY(ix->d_bids.reserve((size_t)H * std::max<uint64_t>(W, 1)));
  FS_HIP(hipMemsetAsync(ix->d_boff.p, 0, (size_t)H * (nb + 1) * sizeof(uint32_t), s));
  if (W) {
    LshDev L = lsh_dev(ix);
    hipLaunchKernelGGL(k_ss, dim3((uint32_t)((W + 255) / 256)), dim3(256), 0, s, ix->d_stok.p,
                       (uint32_t)W, L, ix->d_ss.p, ix->d_sw.p);
    FS_TRY(ix->d_spos.reserve(ix->n_script + FS_MAX_WINDOW));
    FS_HIP(hipMemsetAsync(ix->d_spos.p, 0, (ix->n_script + FS_MAX_WINDOW) * sizeof(fs_spos), s));
    hipLaunchKernelGGL(k_spos, dim3((uint32_t)((ix->n_script + 255) / 256)), dim3(256), 0, s, ix->d_stok.p,
                       (uint32_t)ix->n_script, L, ix->d_spos.p);
    // script window keys and their CSR buckets, all on the device
    DBuf<uint32_t> d_cursor, d_big, d_tmp;
    DBuf<uint32_t>& d_keys = ix->d_skeys;          // (kept: k_lsh_batch compares a window's keys with a script window's)
    FS_TRY(d_keys.reserve(W * H));
    FS_TRY(d_cursor.reserve((size_t)H * nb));
    FS_TRY(d_big.reserve((size_t)H * nb / kSmallBucket + (size_t)H * W / kSmallBucket + 2));
    FS_TRY(d_tmp.reserve((size_t)H * W));
    hipLaunchKernelGGL(k_keys, dim3((uint32_t)std::min<uint64_t>((W + 3) / 4, 4096)), dim3(256), 0,
                       s, L, ix->d_stok.p, (uint32_t)W, d_keys.p);
    const uint32_t gb = (uint32_t)std::min<uint64_t>((W * H + 255) / 256, 4096);
    uint32_t* n_big = d_big.p;                 // [0] = count, list behind it
    FS_HIP(hipMemsetAsync(n_big, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_bucket_count, dim3(gb), dim3(256), 0, s, d_keys.p, (uint32_t)W, H, nb,
                       ix->d_boff.p);
    hipLaunchKernelGGL(k_bucket_offsets, dim3((uint32_t)H), dim3(256), 0, s, nb, ix->d_boff.p,
                       d_cursor.p);
    hipLaunchKernelGGL(k_bucket_fill, dim3(gb), dim3(256), 0, s, d_keys.p, (uint32_t)W, H, nb,
                       d_cursor.p, ix->d_bids.p);
    hipLaunchKernelGGL(k_bucket_sort, dim3((uint32_t)std::min<uint64_t>(((uint64_t)nb * H + 255) / 256, 4096)),
                       dim3(256), 0, s, (uint32_t)W, H, nb, ix->d_boff.p, ix->d_bids.p, d_big.p + 1, n_big);
    hipLaunchKernelGGL(k_bucket_sort_big, dim3(256), dim3(256), 0, s, (uint32_t)W, nb, ix->d_boff.p,
                       ix->d_bids.p, d_big.p + 1, n_big, d_tmp.p);
    FS_HIP(hipGetLastError());
    FS_HIP(hipStreamSynchronize(s));           // the scratch buffers die with this scope
  }
  static_assert(kCntLsh <= FS_LSH_COUNTERS, "fs_index_lsh_counts returns every counter");
  if (ix->sw.lsh_count) {
    FS_TRY(ix->d_lsh_cnt.reserve(2 * FS_LSH_COUNTERS));
    FS_HIP(hipMemsetAsync(ix->d_lsh_cnt.p, 0, FS_LSH_COUNTERS * sizeof(uint64_t), s));
  }
  FS_HIP(hipStreamSynchronize(s));
  ix->lsh_ready = true;
  return FS_OK;
}

int fs_launch_selflev(fs_index* ix, fs_corpus* c, hipStream_t s) {
  const uint32_t W = (uint32_t)ix->n_windows;
  FS_TRY(c->d_selflev.reserve(W + 1));
  if (W) {
    hipLaunchKernelGGL(k_selflev, dim3(std::min<uint32_t>((W + 3) / 4, 4096)), dim3(256), 0, s,
                       ix->gram_dev(), c->dev(), W, c->d_selflev.p);
    FS_HIP(hipGetLastError());
  }
  return FS_OK;
}

// component ids of a batch's tokens (tables with near-synonyms), the scan's pad included
int fs_launch_comp_map(fs_index* ix, fs_corpus* c, hipStream_t s) {
  const uint64_t n = c->n_tok + fs_scan_pad_tokens();
  FS_TRY(c->d_ctok.reserve(n));
  hipLaunchKernelGGL(k_comp_map, dim3(2048), dim3(256), 0, s, (const uint32_t*)c->d_tok.p, (uint32_t)n,
                     (const uint32_t*)ix->d_comp.p, (uint32_t)ix->n_vec, c->d_ctok.p);
  FS_HIP(hipGetLastError());
  return FS_OK;
}
