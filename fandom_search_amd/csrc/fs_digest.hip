// fs_digest.hip -- `ao3.py digest`: the fewest works that show what the fan works quote, greedy
// maximum coverage over the coverage matrix of fs_tiles.h (fs_digest, fs_digest_rows in
// include/fandom_search.h).  K_0 is empty; round r picks the active work with the largest gain
// |C(w) \ K_{r-1}|, the earlier work on a tie, and K_r = K_{r-1} | C(pick); every new word is
// stamped with r.  Afterwards every active work learns how much of it the picks show, the round
// after which they show all of it (its largest stamp) and the pick it shares most words with.
//
// Every output is an integer.  Separate launches; no workgroup waits on another:
//   CoverJob::number / reserve / cover   the passages, the active works, the coverage
//   k_digest_union   a workgroup per tile: the OR of its rows into U, one atomic per wave and word
//   k_digest_total   one workgroup: TOTAL = |U|
//   k_digest_init    a wave per tile: bound := covered, the tile's largest bound, and the best of
//                    round 1, which is the argmax of covered and needs no pass over the matrix
//   k_digest_apply   round r, one workgroup.  A stop rule sets the done word and every later
//                    launch returns at once.  Else the pick's row is ORed into K, its new words
//                    are stamped and their runs walked, every thread a stretch of 64-bit words and
//                    one thread joining the stretches in order, and the pick is written.  Then the
//                    best of round r + 1 is seeded with the recomputed gain of the work that has
//                    the largest stale bound
//   k_digest_gain    round r + 1, a workgroup per tile of 64 active works: a lane is a work, a
//                    wave takes every sixteenth word k, one coalesced 512-byte read each against the
//                    wave-uniform K[k]; gain = sum of popc(row[k] & ~K[k]); the winner is one
//                    64-bit atomic max per tile of gain << 32 | (0xFFFFFFFF - active number)
//   k_digest_gather  the rows of the picks as a matrix of the same layout
//   k_digest_best    a workgroup per tile of active works against every tile of picks
//                    (tile_counts): per work the largest (shared, ~rank)
//   k_digest_works   a workgroup per tile, a lane per work, sixteen waves over the words: its
//                    words in K, its largest stamp when K holds all of them, its fs_digest_work
//
// The lazy bounds.  A work's gain never grows from one round to the next, because K only grows:
// the gain a work had when it was last computed is an upper bound of its gain now, and covered
// is one before round 1.  A tile keeps the largest bound of its works, and k_digest_gain leaves
// a tile unread when that bound is strictly below the gain standing in the round's best.  The
// best is read at agent scope while other workgroups raise it, and that race is sound: within a
// round the best only rises and every value it takes is the true key of some work, so a tile
// is skipped only when each of its works has a true gain <= its bound < a true gain of another
// work; none of them is the round's maximum, nor its equal.  "Strictly" keeps the ties: a tile
// whose bound equals the standing gain may hold an earlier work of the same gain and is read.
// It may, that is, when its works come before the standing one: the test is on the whole key,
// the tile's bound in the high word and its first active number in the low one, which no key
// of the tile exceeds, against the key that stands.  Where many works tie for the largest gain,
// the usual case among thousands of short quotes, only the tiles in front of the first of them
// are read.  The maximum over the tiles that are read is therefore the key of the definition,
// gain and tie-break, whatever the schedule; only the number of tiles read varies.  A work at
// bound 0 is never read again, a tile at bound 0 neither.  FS_DIGEST_LAZY=0 reads every tile
// with a work left in every round and seeds nothing.  The workgroups of a round start together
// while the device has room for them all, so what they see standing is mostly the seed; with
// few tiles the seed is left out (kSeedTiles) and the bounds only spare the tiles at bound 0.
//
// The host enqueues (apply, gain) pairs in batches of FS_DIGEST_BATCH rounds and reads the done
// word and the pick count between batches; it enqueues min(active works, TOTAL, max_picks)
// rounds at most, whatever the device says.
#include "fs_tiles.h"

namespace {

constexpr uint32_t kApply = 256;              // threads of k_digest_apply
constexpr uint32_t kUnionWaves = kBlock / 64;
constexpr uint32_t kGain = 1024;              // threads of k_digest_gain: the words of a tile's
constexpr uint32_t kGainWaves = kGain / 64;   // rows over sixteen waves, a short chain of loads each
constexpr uint32_t kBatch = 64;               // rounds per batch (FS_DIGEST_BATCH)
// The best is seeded above this many tiles (FS_DIGEST_SEED_TILES).  Up to one tile per CU every
// workgroup of k_digest_gain is resident at once: a tile left unread shortens no round, and the
// seed's pass through the apply workgroup only lengthens it (measured: README).
constexpr uint32_t kSeedTiles = 256;

// state[]: what the rounds carry from launch to launch
enum { kDone = 0, kMade = 1, kCum = 2, kTotal = 3, kStateWords = 4 };

struct DigestArgs : CoverArgs {
  uint32_t max_picks, cover, min_gain;
  uint32_t lazy, count;         // FS_DIGEST_LAZY, FS_DIGEST_COUNT
  uint32_t seed;                // the apply pass seeds the next round's best
  uint32_t pick_cap;            // records in picks
  unsigned long long* U;        // [nk] the union of every row
  unsigned long long* K;        // [nk] what the picks so far cover
  uint32_t* stamp;              // [nk * 64] the round a word was first covered in; 0: never
  uint32_t* bound;              // [n_tiles * 64] the gain when it was last computed
  uint32_t* tile_bound;         // [n_tiles] at least the largest bound of the tile
  uint32_t* rank_of;            // [n_tiles * 64] the round an active work was picked in
  unsigned long long* best;     // [1] gain << 32 | (0xFFFFFFFF - active number) of the round
  uint32_t* state;              // [kStateWords]
  unsigned long long* tiles_read;   // [1] tiles k_digest_gain read (FS_DIGEST_COUNT)
  fs_digest_pick* picks;        // [pick_cap]
  uint32_t n_picks, p_tiles;    // picks made, tiles of them
  unsigned long long* prow;     // [p_tiles][nk][64] the rows of the picks
  unsigned long long* wbest;    // [n_tiles * 64] shared << 32 | (0xFFFFFFFF - (rank - 1))
  fs_digest_work* works;
};

__device__ inline const unsigned long long* row_of(const DigestArgs& a, uint32_t ai) {
  return a.cov + (size_t)(ai / kTile) * a.nk * kTile + ai % kTile;
}

// the sum and the maximum over a workgroup of kThreads threads (s_w: kThreads / 64 words of LDS,
// free on return)
template <uint32_t kThreads, class T>
__device__ inline T block_sum(T v, T* s_w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  T tot = 0;
  for (uint32_t w = 0; w < kThreads / 64; ++w) tot += s_w[w];
  __syncthreads();
  return tot;
}

template <uint32_t kThreads, class T>
__device__ inline T block_max(T v, T* s_w) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  T most = 0;
  for (uint32_t w = 0; w < kThreads / 64; ++w)
    if (s_w[w] > most) most = s_w[w];
  __syncthreads();
  return most;
}

__device__ inline unsigned long long wave_or(unsigned long long v) {
  for (uint32_t d = 32; d; d >>= 1) v |= __shfl_xor(v, d);
  return v;
}

// blockIdx.x = tile; wave w takes the words k = w, w + 4, ... (kUnionWaves)
__global__ __launch_bounds__(kBlock) void k_digest_union(DigestArgs a) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* row = a.cov + (size_t)blockIdx.x * a.nk * kTile + lane;
  for (uint32_t k = wave; k < a.nk; k += kUnionWaves) {
    const unsigned long long u = wave_or(row[(size_t)k * kTile]);
    if (u && lane == 0) atomicOr(&a.U[k], u);
  }
}

__global__ __launch_bounds__(kApply) void k_digest_total(DigestArgs a) {
  __shared__ uint32_t s_w[kApply / 64];
  uint32_t c = 0;
  for (uint32_t k = threadIdx.x; k < a.nk; k += kApply) c += (uint32_t)__popcll(a.U[k]);
  c = block_sum<kApply>(c, s_w);
  if (threadIdx.x == 0) a.state[kTotal] = c;
}

// blockIdx.x = tile, a lane per work (rows past the last active work cover nothing)
__global__ __launch_bounds__(kTile) void k_digest_init(DigestArgs a) {
  const uint32_t ai = blockIdx.x * kTile + threadIdx.x;
  const uint32_t c = a.covered[ai];
  a.bound[ai] = c;
  a.rank_of[ai] = FS_NONE;
  const uint32_t most = wave_max(c);
  const unsigned long long key =
      wave_max(c ? ((unsigned long long)c << 32) | (0xFFFFFFFFu - ai) : 0ull);
  if (threadIdx.x == 0) {
    a.tile_bound[blockIdx.x] = most;
    if (key) atomicMax(a.best, key);
  }
}

// The runs of ones in the 64-bit words x of a stretch, in order: word(x, base) per word, base
// its first bit's index; closed(start, length) for every run that ends inside the stretch; the
// run that reaches the stretch's last bit stays open in (cur_s, cur_n).  The walk of
// k_pairs_detail (fs_pairs.hip), its best run left to the caller.
struct RunWalk {
  uint32_t cur_s = 0, cur_n = 0;
  template <class Closed>
  __device__ void word(unsigned long long x, uint32_t base, Closed closed) {
    if (x == 0) {
      if (cur_n) closed(cur_s, cur_n);
      cur_n = 0;
      return;
    }
    if (x == ~0ull) {
      if (!cur_n) cur_s = base;
      cur_n += 64;
      return;
    }
    const uint32_t t = (uint32_t)__builtin_ctzll(~x);      // ones from bit 0 on: the open run goes on
    if (t) {
      if (!cur_n) cur_s = base;
      cur_n += t;
      x &= ~0ull << t;
    }
    if (cur_n) closed(cur_s, cur_n);
    cur_n = 0;
    while (x) {
      const uint32_t s = (uint32_t)__builtin_ctzll(x);     // s >= 1: bit t is clear
      const uint32_t l = (uint32_t)__builtin_ctzll(~(x >> s));
      if (s + l == 64) {                                   // up to the word's last bit: left open
        cur_s = base + s;
        cur_n = l;
        break;
      }
      closed(base + s, l);
      x &= ~0ull << (s + l);
    }
  }
};

// One workgroup: round r = state[kMade] + 1 from the best the launches before left.  What does
// not wait for the pick is loaded beside it: the tiles' bounds for the seed, the bounds of the
// seed's tile beside the pick's row.
__global__ __launch_bounds__(kApply) void k_digest_apply(DigestArgs a) {
  // per thread, the new words of its stretch: the run from its first bit (s_pre words; s_full: it
  // is the whole stretch), the open run at its end, the longest run strictly inside, the runs
  // closed inside other than the first; s_some: the stretches of a wave that hold a new word
  __shared__ uint32_t s_pre[kApply], s_full[kApply], s_suf_s[kApply], s_suf_n[kApply];
  __shared__ uint32_t s_in_s[kApply], s_in_n[kApply], s_runs[kApply];
  __shared__ unsigned long long s_some[kApply / 64];
  __shared__ uint32_t s_w[kApply / 64];
  __shared__ unsigned long long s_w64[kApply / 64];
  __shared__ uint32_t s_pick, s_round, s_seed;
  const uint32_t tid = threadIdx.x;
  uint32_t cum = 0;
  if (tid == 0) {
    uint32_t pick = FS_NONE;
    const uint32_t made = a.state[kMade];
    cum = a.state[kCum];
    if (!a.state[kDone]) {
      const unsigned long long b = *a.best;
      const uint32_t gain = (uint32_t)(b >> 32);
      const bool stop = gain < a.min_gain || (a.max_picks && made >= a.max_picks) ||
                        made >= a.pick_cap ||
                        (unsigned long long)cum * 100ull >=
                            (unsigned long long)a.cover * a.state[kTotal];
      if (stop)
        a.state[kDone] = 1u;
      else
        pick = 0xFFFFFFFFu - (uint32_t)b;
    }
    s_pick = pick;
    s_round = made + 1;
  }
  // the seed's tile: the largest bound, the first tile among equals
  unsigned long long top = 0;
  if (a.seed) {
    for (uint32_t t = tid; t < a.n_tiles; t += kApply) {
      const unsigned long long key =
          ((unsigned long long)a.tile_bound[t] << 32) | (0xFFFFFFFFu - t);
      if (key > top) top = key;
    }
  }
  top = block_max<kApply>(top, s_w64);                     // (and s_pick is written)
  const uint32_t ai = s_pick;
  if (ai >= a.n_active) return;                            // done, or (never) no such work
  const uint32_t r = s_round;
  const uint32_t seed_tile = 0xFFFFFFFFu - (uint32_t)top;  // (top >> 32 != 0: a tile)
  uint32_t seed_bound = 0, wk = 0, cv = 0;
  if ((top >> 32) && tid < kTile && seed_tile * kTile + tid != ai)
    seed_bound = a.bound[seed_tile * kTile + tid];         // (the pick's own becomes 0)
  if (tid == 0) {
    wk = a.work_of[ai];
    cv = a.covered[ai];
  }
  const unsigned long long* row = row_of(a, ai);
  const uint32_t per = (a.nk + kApply - 1) / kApply;
  const uint32_t k0 = tid * per < a.nk ? tid * per : a.nk;
  const uint32_t k1 = a.nk - k0 < per ? a.nk : k0 + per;
  const uint32_t start = k0 * 64;
  RunWalk walk;
  uint32_t fresh = 0, pre = 0, in_s = 0, in_n = 0, runs = 0;
  auto closed = [&](uint32_t s, uint32_t n) {
    if (s == start) {
      pre = n;
    } else {
      ++runs;
      if (n > in_n) { in_n = n; in_s = s; }
    }
  };
  for (uint32_t k = k0; k < k1; ++k) {
    const unsigned long long x = row[(size_t)k * kTile], was = a.K[k];
    unsigned long long nw = x & ~was;
    if (nw) a.K[k] = was | x;
    fresh += (uint32_t)__popcll(nw);
    walk.word(nw, k * 64, closed);
    while (nw) {
      a.stamp[k * 64 + (uint32_t)__builtin_ctzll(nw)] = r;
      nw &= nw - 1;
    }
  }
  const bool full = k1 > k0 && walk.cur_n == (k1 - k0) * 64;
  s_pre[tid] = full ? walk.cur_n : pre;
  s_full[tid] = full;
  s_suf_s[tid] = walk.cur_s;
  s_suf_n[tid] = full ? 0u : walk.cur_n;
  s_in_s[tid] = in_s;
  s_in_n[tid] = in_n;
  s_runs[tid] = runs;
  const unsigned long long some = __ballot(fresh != 0);
  if ((tid & 63) == 0) s_some[tid >> 6] = some;
  fresh = block_sum<kApply>(fresh, s_w);                   // (and the tables above are written)
  if (tid < kTile) {                                       // the work of the largest bound there
    const unsigned long long key = wave_max(
        seed_bound ? ((unsigned long long)seed_bound << 32) | (0xFFFFFFFFu - tid) : 0ull);
    if (tid == 0) {
      s_seed = key ? seed_tile * kTile + (0xFFFFFFFFu - (uint32_t)key) : FS_NONE;
      if (top >> 32) a.tile_bound[seed_tile] = (uint32_t)(key >> 32);   // (still above its bounds)
    }
  }
  if (tid == 0) {
    // the stretches with a new word in order; a stretch without one in between closes the open
    // run.  The open run goes on through a full stretch, else it takes the stretch's first run
    // and closes in front of the runs inside; a later run replaces the best only when it is
    // longer
    uint32_t cur_s = 0, cur_n = 0, best_s = 0, best_n = 0, n_runs = 0, next = 0;
    for (uint32_t w = 0; w < kApply / 64; ++w) {
      unsigned long long m = s_some[w];
      while (m) {
        const uint32_t c = w * 64 + (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        if (c != next && cur_n) {                          // (a stretch without a new word)
          ++n_runs;
          if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
          cur_n = 0;
        }
        next = c + 1;
        if (s_full[c]) {
          if (!cur_n) cur_s = c * per * 64;
          cur_n += s_pre[c];
          continue;
        }
        if (s_pre[c]) {
          if (!cur_n) cur_s = c * per * 64;
          cur_n += s_pre[c];
        }
        if (cur_n) {
          ++n_runs;
          if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
        }
        n_runs += s_runs[c];
        if (s_in_n[c] > best_n) { best_n = s_in_n[c]; best_s = s_in_s[c]; }
        cur_s = s_suf_s[c];
        cur_n = s_suf_n[c];
      }
    }
    if (cur_n) {
      ++n_runs;
      if (cur_n > best_n) { best_n = cur_n; best_s = cur_s; }
    }
    cum += fresh;
    uint4* p = reinterpret_cast<uint4*>(a.picks + (r - 1));
    p[0] = make_uint4(wk, cv, fresh, n_runs);
    p[1] = make_uint4(best_s, best_n, cum, 0u);
    a.state[kMade] = r;
    a.state[kCum] = cum;
    a.rank_of[ai] = r;
    a.bound[ai] = 0u;
    *a.best = 0ull;                                        // the next round's, unless seeded below
  }
  if (!a.seed) return;
  __syncthreads();                                         // s_seed is written
  // the seed's gain against the new K, every thread the words it has just written itself
  const uint32_t seed = s_seed;
  if (seed >= a.n_active) return;
  const unsigned long long* srow = row_of(a, seed);
  uint32_t g = 0;
  for (uint32_t k = k0; k < k1; ++k) g += (uint32_t)__popcll(srow[(size_t)k * kTile] & ~a.K[k]);
  g = block_sum<kApply>(g, s_w);
  if (tid == 0) {
    a.bound[seed] = g;
    if (g) *a.best = ((unsigned long long)g << 32) | (0xFFFFFFFFu - seed);
  }
}

// blockIdx.x = tile; a lane is a work, wave w takes the words k = w, w + 16, ...
__global__ __launch_bounds__(kGain) void k_digest_gain(DigestArgs a) {
  __shared__ uint32_t s_go;
  __shared__ unsigned long long s_seen;
  __shared__ uint32_t s_g[kGainWaves][kTile];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x == 0) {
    uint32_t go = 0;
    unsigned long long seen = 0;
    if (!a.state[kDone]) {
      const uint32_t tb = a.tile_bound[blockIdx.x];
      // what stands in the best, past the vector cache, against the best this tile could give:
      // its bound in its first work
      seen = __hip_atomic_load(a.best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long most =
          ((unsigned long long)tb << 32) | (0xFFFFFFFFu - blockIdx.x * kTile);
      go = tb != 0 && (!a.lazy || most > seen);
    }
    s_go = go;
    s_seen = seen;
  }
  __syncthreads();
  if (!s_go) return;
  const uint32_t ai = blockIdx.x * kTile + lane;
  const unsigned long long* row = a.cov + (size_t)blockIdx.x * a.nk * kTile + lane;
  uint32_t g = 0;
  if (a.bound[ai]) {
#pragma unroll 4
    for (uint32_t k = wave; k < a.nk; k += kGainWaves)
      g += (uint32_t)__popcll(row[(size_t)k * kTile] & ~a.K[k]);
  }
  s_g[wave][lane] = g;
  __syncthreads();
  if (wave) return;
  g = 0;
#pragma unroll
  for (uint32_t w = 0; w < kGainWaves; ++w) g += s_g[w][lane];
  a.bound[ai] = g;
  const unsigned long long key =
      wave_max(g ? ((unsigned long long)g << 32) | (0xFFFFFFFFu - ai) : 0ull);
  if (lane == 0) {
    a.tile_bound[blockIdx.x] = (uint32_t)(key >> 32);
    // (at or below what was seen the maximum changes nothing: the best only rises)
    if (key > s_seen) atomicMax(a.best, key);
    if (a.count) atomicAdd(a.tiles_read, 1ull);
  }
}

// a lane per word of the picks' matrix: [pick tile][k][pick of the tile]
__global__ __launch_bounds__(kRunBlock) void k_digest_gather(DigestArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * kRunBlock + threadIdx.x;
  if (i >= (uint64_t)a.p_tiles * a.nk * kTile) return;
  const uint32_t p = (uint32_t)(i / ((uint64_t)a.nk * kTile)) * kTile + (uint32_t)(i % kTile);
  const uint32_t k = (uint32_t)((i / kTile) % a.nk);
  unsigned long long x = 0;
  if (p < a.n_picks) x = row_of(a, a.act[a.picks[p].work])[(size_t)k * kTile];
  a.prow[i] = x;
}

// blockIdx.x = tile of active works, against every tile of picks in rank order
__global__ __launch_bounds__(kBlock) void k_digest_best(DigestArgs a) {
  __shared__ __align__(16) unsigned long long s_a[kSlice * kTile];
  __shared__ __align__(16) unsigned long long s_b[kSlice * kTile];
  __shared__ uint32_t s_sh[kTile * kShStride];
  __shared__ unsigned long long s_best[kTile];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < kTile) s_best[threadIdx.x] = 0ull;
  const unsigned long long* ga = a.cov + (size_t)blockIdx.x * a.nk * kTile;
  for (uint32_t pj = 0; pj < a.p_tiles; ++pj) {
    __syncthreads();                                       // s_sh of the tile before
    tile_counts(ga, a.prow + (size_t)pj * a.nk * kTile, a.nk, s_a, s_b, s_sh);
    // rows: wave w takes rows 16 w .. 16 w + 15 (and is the only one to), a lane per pick
    const uint32_t p = pj * kTile + lane;
    for (uint32_t rr = 0; rr < kTile / 4; ++rr) {
      const uint32_t r = wave * (kTile / 4) + rr;
      const uint32_t sh = s_sh[r * kShStride + lane];
      const unsigned long long key = wave_max(
          sh && p < a.n_picks ? ((unsigned long long)sh << 32) | (0xFFFFFFFFu - p) : 0ull);
      if (lane == 0 && key > s_best[r]) s_best[r] = key;
    }
  }
  __syncthreads();
  if (threadIdx.x < kTile) a.wbest[(size_t)blockIdx.x * kTile + threadIdx.x] = s_best[threadIdx.x];
}

// blockIdx.x = tile; a lane is a work, wave w takes the words k = w, w + 16, ...: its words in
// K, whether K lacks one, the largest stamp of those it holds
__global__ __launch_bounds__(kGain) void k_digest_works(DigestArgs a) {
  __shared__ uint32_t s_in[kGainWaves][kTile], s_at[kGainWaves][kTile], s_miss[kGainWaves][kTile];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t ai = blockIdx.x * kTile + lane;
  const unsigned long long* row = a.cov + (size_t)blockIdx.x * a.nk * kTile + lane;
  uint32_t in = 0, at = 0, miss = 0;
  for (uint32_t k = wave; k < a.nk; k += kGainWaves) {
    const unsigned long long x = row[(size_t)k * kTile], kk = a.K[k];
    unsigned long long y = x & kk;
    in += (uint32_t)__popcll(y);
    miss |= (x & ~kk) != 0;
    while (y) {
      const uint32_t s = a.stamp[k * 64 + (uint32_t)__builtin_ctzll(y)];
      if (s > at) at = s;
      y &= y - 1;
    }
  }
  s_in[wave][lane] = in;
  s_at[wave][lane] = at;
  s_miss[wave][lane] = miss;
  __syncthreads();
  if (wave || ai >= a.n_active) return;
  in = at = miss = 0;
  for (uint32_t w = 0; w < kGainWaves; ++w) {
    in += s_in[w][lane];
    miss |= s_miss[w][lane];
    if (s_at[w][lane] > at) at = s_at[w][lane];
  }
  const unsigned long long b = a.wbest[ai];
  uint4* p = reinterpret_cast<uint4*>(a.works + ai);
  p[0] = make_uint4(a.work_of[ai], a.covered[ai], a.rank_of[ai], in);
  p[1] = make_uint4(miss ? FS_NONE : at, b ? 0xFFFFFFFFu - (uint32_t)b + 1u : FS_NONE,
                    (uint32_t)(b >> 32), 0u);
}

// coverage, rounds, works, their total; then what the rounds did: rounds enqueued, tiles read
thread_local double t_ms[6];

// one call: rounds() through the picks, then write()
struct DigestJob {
  CoverJob cj;
  DBuf<unsigned long long> words, best, wbest, prow, tiles_read;
  DBuf<uint32_t> stamp, per_work, tile_bound, state;
  DBuf<fs_digest_pick> picks;
  Clock<4> clk;
  DigestArgs a{};
  uint32_t n_picks = 0, total = 0;

  // a.n_active, n_picks, total and the picks on the device set (all on `s`, finished on return)
  int rounds(const fs_row* d_rows, uint32_t n, uint32_t n_works, uint32_t n_script,
             uint32_t min_words, uint32_t max_gap, uint32_t max_picks, uint32_t cover,
             uint32_t min_gain, hipStream_t s) {
    for (double& t : t_ms) t = 0.0;
    a.n = n;
    a.n_works = n_works;
    a.n_script = n_script;
    a.nk = (n_script + 63) / 64;
    a.min_words = min_words;
    a.max_picks = max_picks;
    a.cover = cover;
    a.min_gain = min_gain;
    a.lazy = env_u32("FS_DIGEST_LAZY", 1u, 1u);
    a.count = env_u32("FS_DIGEST_COUNT", 0u, 1u);
    uint32_t batch = env_u32("FS_DIGEST_BATCH", kBatch, 1u << 16);
    if (!batch) batch = kBatch;
    const uint64_t max_bytes = FS_DIGEST_MAX_BYTES;
    if (!n) return FS_OK;
    FS_TRY(cj.number(d_rows, a, max_gap, s));
    if (!a.n_active) return FS_OK;
    a.seed = a.lazy && a.n_tiles > env_u32("FS_DIGEST_SEED_TILES", kSeedTiles, 0xFFFFFFFFu);
    const size_t rows = (size_t)a.n_tiles * kTile;
    // no more picks than active works, than script words, than the caller allows
    uint32_t most = a.n_active < n_script ? a.n_active : n_script;
    if (max_picks && max_picks < most) most = max_picks;
    const uint64_t cov_bytes = (uint64_t)rows * a.nk * 8;
    const uint64_t pick_bytes = (uint64_t)((most + kTile - 1) / kTile) * kTile * a.nk * 8;
    const uint64_t work_bytes = (uint64_t)rows * 16 + (uint64_t)a.nk * (16 + 256) +
                                (uint64_t)most * sizeof(fs_digest_pick);
    if (cov_bytes + pick_bytes + work_bytes > max_bytes) {
      fs_set_error("%u works with a passage over %u script words: a coverage matrix of %llu "
                   "bytes, the rows of up to %u picks gathered for the best-pick pass (%llu "
                   "bytes) and the arrays per work, word and pick (%llu bytes) are more than "
                   "%llu bytes", a.n_active, n_script, (unsigned long long)cov_bytes, most,
                   (unsigned long long)pick_bytes, (unsigned long long)work_bytes,
                   (unsigned long long)max_bytes);
      return FS_E_UNSUPPORTED;
    }
    FS_TRY(cj.reserve(a, s));
    FS_TRY(words.reserve(2 * (size_t)a.nk));
    FS_TRY(stamp.reserve((size_t)a.nk * 64));
    FS_TRY(per_work.reserve(2 * rows));
    FS_TRY(tile_bound.reserve(a.n_tiles));
    FS_TRY(best.reserve(1));
    FS_TRY(tiles_read.reserve(1));
    FS_TRY(state.reserve(kStateWords));
    FS_TRY(picks.reserve(most));
    FS_HIP(hipMemsetAsync(words.p, 0, 2 * (size_t)a.nk * sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(stamp.p, 0, (size_t)a.nk * 64 * sizeof(uint32_t), s));
    FS_HIP(hipMemsetAsync(best.p, 0, sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(tiles_read.p, 0, sizeof(unsigned long long), s));
    FS_HIP(hipMemsetAsync(state.p, 0, kStateWords * sizeof(uint32_t), s));
    a.U = words.p;
    a.K = words.p + a.nk;
    a.stamp = stamp.p;
    a.bound = per_work.p;
    a.rank_of = per_work.p + rows;
    a.tile_bound = tile_bound.p;
    a.best = best.p;
    a.tiles_read = tiles_read.p;
    a.state = state.p;
    a.picks = picks.p;
    a.pick_cap = most;
    FS_TRY(clk.mark(0, s));
    cj.cover(d_rows, a, s);
    hipLaunchKernelGGL(k_digest_union, dim3(a.n_tiles), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_digest_total, dim3(1), dim3(kApply), 0, s, a);
    hipLaunchKernelGGL(k_digest_init, dim3(a.n_tiles), dim3(kTile), 0, s, a);
    FS_TRY(clk.mark(1, s));
    FS_HIP(hipGetLastError());
    uint32_t st[kStateWords] = {};
    FS_HIP(hipMemcpyAsync(st, state.p, sizeof st, hipMemcpyDeviceToHost, s));
    FS_HIP(hipStreamSynchronize(s));
    total = st[kTotal];
    if (total < most) most = total;                        // every pick has a new word
    // the rounds: bounded by `most` here, whatever the done word says
    uint32_t enqueued = 0;
    while (enqueued < most && !st[kDone]) {
      const uint32_t now = most - enqueued < batch ? most - enqueued : batch;
      for (uint32_t r = 0; r < now; ++r) {
        hipLaunchKernelGGL(k_digest_apply, dim3(1), dim3(kApply), 0, s, a);
        if (enqueued + r + 1 < most)                       // (behind the last pick: no round)
          hipLaunchKernelGGL(k_digest_gain, dim3(a.n_tiles), dim3(kGain), 0, s, a);
      }
      enqueued += now;
      FS_HIP(hipGetLastError());
      FS_HIP(hipMemcpyAsync(st, state.p, sizeof st, hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
    }
    FS_TRY(clk.mark(2, s));
    n_picks = st[kMade] < most ? st[kMade] : most;
    t_ms[4] = (double)enqueued;
    if (a.count) {
      unsigned long long read = 0;
      FS_HIP(hipMemcpyAsync(&read, tiles_read.p, sizeof read, hipMemcpyDeviceToHost, s));
      FS_HIP(hipStreamSynchronize(s));
      t_ms[5] = (double)read;
    }
    return FS_OK;
  }

  // the n_picks picks into d_picks (unless it is the job's own buffer) and the a.n_active works
  // into d_works (finished on return)
  int write(fs_digest_pick* d_picks, fs_digest_work* d_works, hipStream_t s) {
    if (!a.n_active) return FS_OK;
    const size_t rows = (size_t)a.n_tiles * kTile;
    a.n_picks = n_picks;
    a.p_tiles = (n_picks + kTile - 1) / kTile;
    a.works = d_works;
    FS_TRY(wbest.reserve(rows));
    FS_TRY(prow.reserve((size_t)a.p_tiles * a.nk * kTile));
    a.wbest = wbest.p;
    a.prow = prow.p;
    const uint64_t cells = (uint64_t)a.p_tiles * a.nk * kTile;
    if (cells) hipLaunchKernelGGL(k_digest_gather, dim3(blocks_of(cells, kRunBlock)),
                                  dim3(kRunBlock), 0, s, a);
    hipLaunchKernelGGL(k_digest_best, dim3(a.n_tiles), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL(k_digest_works, dim3(a.n_tiles), dim3(kGain), 0, s, a);
    FS_TRY(clk.mark(3, s));
    FS_HIP(hipGetLastError());
    if (n_picks && d_picks != picks.p)
      FS_HIP(hipMemcpyAsync(d_picks, picks.p, (size_t)n_picks * sizeof(fs_digest_pick),
                            hipMemcpyDeviceToDevice, s));
    FS_HIP(hipStreamSynchronize(s));
    t_ms[0] = clk.elapsed(0, 1);
    t_ms[1] = clk.elapsed(1, 2);
    t_ms[2] = clk.elapsed(2, 3);
    t_ms[3] = t_ms[0] + t_ms[1] + t_ms[2];
    return FS_OK;
  }
};

// the rules both entry points share
int digest_check(uint64_t n_rows, uint32_t n_script, uint32_t min_words, uint32_t cover,
                 uint32_t min_gain, const void* picks, uint64_t picks_cap, uint64_t* n_picks,
                 const void* works, uint64_t works_cap, uint64_t* n_active,
                 uint64_t* total_words) {
  if (!n_picks || !n_active || !total_words || (picks_cap && !picks) || (works_cap && !works)) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (min_words == 0 || min_gain == 0) {
    fs_set_error("min_words and min_gain must be at least 1");
    return FS_E_INVALID;
  }
  if (cover == 0 || cover > 100) {
    fs_set_error("cover %u: a whole percentage from 1 to 100", cover);
    return FS_E_INVALID;
  }
  FS_TRY(record_limits("digests", n_rows, n_script));
  *n_picks = 0;
  *n_active = 0;
  *total_words = 0;
  return FS_OK;
}

}  // namespace

extern "C" int fs_digest(int device, const uint32_t* work, const uint32_t* fan_ix,
                         const uint32_t* orig_ix, uint64_t n_rows, uint32_t n_works,
                         uint32_t n_script, uint32_t min_words, uint32_t max_gap,
                         uint32_t max_picks, uint32_t cover, uint32_t min_gain,
                         fs_digest_pick* picks, uint64_t picks_cap, uint64_t* n_picks,
                         fs_digest_work* works, uint64_t works_cap, uint64_t* n_active,
                         uint64_t* total_words) {
  FS_TRY(digest_check(n_rows, n_script, min_words, cover, min_gain, picks, picks_cap, n_picks,
                      works, works_cap, n_active, total_words));
  if (!n_rows) return FS_OK;
  if (!work || !fan_ix || !orig_ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  FS_ENTER(device);
  const uint32_t n = (uint32_t)n_rows;
  DBuf<fs_row> rows;
  DBuf<fs_digest_work> d_works;
  FS_TRY(fs_host_rows(rows, work, fan_ix, orig_ix, n));
  DigestJob job;
  FS_TRY(job.rounds(rows.p, n, n_works, n_script, min_words, max_gap, max_picks, cover, min_gain,
                    nullptr));
  *n_picks = job.n_picks;
  *n_active = job.a.n_active;
  *total_words = job.total;
  if (job.n_picks > picks_cap || job.a.n_active > works_cap) return FS_E_CAPACITY;
  if (!job.a.n_active) return FS_OK;
  FS_TRY(d_works.reserve(job.a.n_active));
  FS_TRY(job.write(job.picks.p, d_works.p, nullptr));
  if (job.n_picks) FS_TRY(copy_out(picks, job.picks, job.n_picks));
  FS_TRY(copy_out(works, d_works, job.a.n_active));
  FS_HIP(hipDeviceSynchronize());
  return FS_OK;
}

extern "C" int fs_digest_rows(fs_index* ix, const fs_row* d_rows, uint64_t n_rows,
                              uint32_t n_works, uint32_t min_words, uint32_t max_gap,
                              uint32_t max_picks, uint32_t cover, uint32_t min_gain,
                              fs_digest_pick* d_picks, uint64_t picks_cap, uint64_t* n_picks,
                              fs_digest_work* d_works, uint64_t works_cap, uint64_t* n_active,
                              uint64_t* total_words) {
  if (!ix) {
    fs_set_error("null argument");
    return FS_E_INVALID;
  }
  if (ix->n_script > FS_WORKS_MAX_SCRIPT) {
    fs_set_error("a script of %llu words: digests take up to %u",
                 (unsigned long long)ix->n_script, FS_WORKS_MAX_SCRIPT);
    return FS_E_UNSUPPORTED;
  }
  FS_TRY(digest_check(n_rows, (uint32_t)ix->n_script, min_words, cover, min_gain, d_picks,
                      picks_cap, n_picks, d_works, works_cap, n_active, total_words));
  if ((n_rows && (!d_rows || ((uintptr_t)d_rows & 15))) || ((uintptr_t)d_picks & 15) ||
      ((uintptr_t)d_works & 15)) {
    fs_set_error("d_rows, d_picks and d_works must be 16-byte aligned device pointers");
    return FS_E_INVALID;
  }
  if (!n_rows) return FS_OK;
  FS_ENTER(ix->device);
  DigestJob job;
  FS_TRY(job.rounds(d_rows, (uint32_t)n_rows, n_works, (uint32_t)ix->n_script, min_words, max_gap,
                    max_picks, cover, min_gain, ix->stream));
  *n_picks = job.n_picks;
  *n_active = job.a.n_active;
  *total_words = job.total;
  if (job.n_picks > picks_cap || job.a.n_active > works_cap) return FS_E_CAPACITY;
  return job.write(d_picks, d_works, ix->stream);
}

extern "C" int fs_digest_times(double* ms) {
  return times_out(ms, t_ms, 6);
}
