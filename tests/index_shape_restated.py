"""The size rules of the script index and of the k_scan_rows launch, restated in plain Python
(test helper, no GPU).

The index build (build_gram_index, fs_api.hip) and the launch (fs_scan_rows_shape,
fs_scan_rows_disp_lds, rows_filter_log2, fs_scan.hip) choose buffer sizes, kernel instances,
launch shapes and the record form by the script's length S and its number of distinct n-grams
G.  Every rule is written here a second time, from the formulas, so that a test can say on the
CPU which side of an edge a script lies on before the GPU is asked (ScriptIndex.scan_shape).
The hash of an n-gram, its bucket and the sub-shingle filter (fs_hash.h) are restated too: a
test can then plant a quote whose n-gram falls into a chosen bucket, and count on the CPU how
many windows of a batch the filter lets through.
"""

import math

import numpy as np

PACKED8_BITS = 18                 # an 8-byte record holds orig_ix in 18 bits, k in 4, lev in 10
CU_LDS_BYTES = 160 * 1024         # LDS of a gfx950 CU: the most one workgroup may ask for
SEEDS_LDS_MAX = 16 * 1024         # displacement seeds as bytes: in LDS up to this many

# sizeof(FusedLds), the per-wave LDS of k_scan_rows (fs_scan.hip, fs_ranges.h):
#   RangeLds: 72 hits of 16 bytes, 64 {work, first token} of 8, 64 words, 512 owner bytes
#   the wave's queue of 192 records and the 64 positions of the round being made up
RANGE_LDS = 72 * 16 + 64 * 8 + 64 * 4 + 64 * 8
FUSED_LDS = RANGE_LDS + 192 * 4 + 64 * 4
# sizeof(CoopLds), the shared rounds' LDS of a workgroup (fs_ranges.h): 96 slices of ten words,
# a ring of 96 + 16 words, four counters, sixteen words of statistics
COOP_LDS = 96 * 40 + (96 + 16) * 4 + 4 * 4 + 16 * 4
COUNTERS_LDS = 1024               # s_cnt and the slices of the shared rounds


def ceil_log2(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def host_wire8(n_script):
    """A host search of the exact pipeline brings 8-byte records over; fs_rows_unpack8 and
    FS_ROWS_DEVICE_PACKED8 are refused from the same length on."""
    return n_script < (1 << PACKED8_BITS)


def bloom_log2_words(G):
    """Bloom filter of the chained kernels: about one word per n-gram, 2^10 .. 2^15 words."""
    return min(15, max(10, ceil_log2(max(1, G * 3 // 4))))


def sub_k(n):
    return 4 if n >= 6 else 3 if n >= 4 else 0


def sub_words_wanted(n_script, n):
    """Words of the sub-shingle filter before the clamp: bit density 0.002^(1 / (n - K + 1))."""
    dens = math.pow(2e-3, 1.0 / (n - sub_k(n) + 1))
    return int(max(1, n_script) / (32.0 * dens)) + 1


def sub_log2_words(n_script, n):
    return min(14, max(10, ceil_log2(sub_words_wanted(n_script, n))))


def log2_slots(G):
    """Exact table: at most half full."""
    return max(4, ceil_log2(G * 2 + 1))


def log2_buckets(G):
    """Hash-and-displace: about four n-grams per bucket."""
    return max(2, ceil_log2(max(1, G // 4)))


def seeds_lds_bytes(G, disp_lds=True):
    """Bytes of displacement seeds k_scan_rows holds in LDS; 0: it reads them from memory."""
    nbytes = ((1 << log2_buckets(G)) + 15) & ~15
    return nbytes if nbytes <= SEEDS_LDS_MAX and disp_lds else 0


def rows_filter_log2(n_script, G, n, scan_sub=True):
    """log2 words of the filter k_scan_rows holds in LDS."""
    return sub_log2_words(n_script, n) if sub_k(n) and scan_sub else bloom_log2_words(G)


def rows_fixed_lds(n_script, G, n):
    """LDS of a k_scan_rows workgroup beside its per-wave state."""
    return (4 << rows_filter_log2(n_script, G, n)) + seeds_lds_bytes(G) + COUNTERS_LDS + COOP_LDS


def rows_waves(n_script, G, n, lanes):
    """(waves per workgroup, workgroups per CU) of k_scan_rows on a batch small enough for any
    shape: two workgroups of eight per CU when searches overlap (several lanes) and the LDS
    takes them twice, else one workgroup of the most waves that fit."""
    fixed = rows_fixed_lds(n_script, G, n)
    if lanes > 1 and 2 * (fixed + 8 * FUSED_LDS) <= CU_LDS_BYTES:
        return 8, 2
    for w in (16, 8, 4):
        if fixed + w * FUSED_LDS <= CU_LDS_BYTES:
            return w, 1
    return 0, 0


# ---- fs_hash.h -----------------------------------------------------------------------------

TOKEN_MUL24 = 0x9E3779
U32 = 0xFFFFFFFF


def premix(tok):
    return ((np.asarray(tok, dtype=np.uint64) & np.uint64(0xFFFFFF)) * np.uint64(TOKEN_MUL24)) & np.uint64(U32)


def rotl(x, r):
    r &= 31
    x = np.asarray(x, dtype=np.uint64)
    if r == 0:
        return x
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & np.uint64(U32)


def gram_hash(tokens, n):
    """fs_gram_hash of every window of `tokens` (uint64 array of 32-bit values)."""
    m = premix(tokens)
    W = len(m) - n + 1
    x = np.zeros(max(W, 0), dtype=np.uint64)
    for k in range(n):
        x ^= rotl(m[k:k + W], 7 * (n - 1 - k))
    return x


def table_bucket(h, log2_b):
    h = np.asarray(h, dtype=np.uint64)
    return ((h * np.uint64(0x85EBCA6B)) & np.uint64(U32)) >> np.uint64(32 - log2_b)


def gram_hash_one(ids):
    """The same hash of one n-gram in plain Python integers."""
    x, n = 0, len(ids)
    for k, t in enumerate(ids):
        m = ((int(t) & 0xFFFFFF) * TOKEN_MUL24) & U32
        r = (7 * (n - 1 - k)) & 31
        x ^= ((m << r) | (m >> ((32 - r) & 31))) & U32 if r else m
    return x


def distinct_grams(tokens, n):
    """G: the number of distinct n-grams of a script (fs_index_info.n_grams)."""
    if len(tokens) < n:
        return 0
    return len(np.unique(np.lib.stride_tricks.sliding_window_view(np.asarray(tokens), n), axis=0))


def _window_keys(tokens, n):
    w = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(np.asarray(tokens, dtype=np.uint32), n))
    return w.view(np.dtype((np.void, 4 * n))).reshape(-1)


def matching_windows(work, script, n):
    """Windows of one fan work whose n ids are a script n-gram: the true candidates."""
    if len(work) < n or len(script) < n:
        return 0
    return int(np.isin(_window_keys(work, n), np.unique(_window_keys(script, n))).sum())


def sub_hash(tokens, K):
    """fs_sub_hash of every K-gram: a polynomial in 2^S of the premixed ids, modulo 2^32."""
    S = 8 if K >= 4 else 11
    m = premix(tokens)
    W = len(m) - K + 1
    x = np.zeros(max(W, 0), dtype=np.uint64)
    for k in range(K):
        x = ((x << np.uint64(S)) + m[k:k + W]) & np.uint64(U32)
    return x


def sub_filter(script, n, log2_w=None):
    """The sub-shingle filter of a script: one bit per script K-gram."""
    K = sub_k(n)
    lw = sub_log2_words(len(script), n) if log2_w is None else log2_w
    h = sub_hash(script, K)
    words = np.zeros(1 << lw, dtype=np.uint32)
    np.bitwise_or.at(words, ((h >> np.uint64(18)) & np.uint64((1 << lw) - 1)).astype(np.int64),
                     (np.uint32(1) << ((h >> np.uint64(8)) & np.uint64(31)).astype(np.uint32)))
    return words


def sub_filter_density(words):
    return float(np.unpackbits(words.view(np.uint8)).sum()) / (32.0 * len(words))


def sub_pass_count(work, script, n):
    """Windows of one fan work that the sub-shingle filter lets through: all n - K + 1 of
    their K-grams are set.  These are the candidates of k_scan_rows on that work."""
    K = sub_k(n)
    words = sub_filter(script, n)
    lw = ceil_log2(len(words))
    h = sub_hash(work, K)
    bit = (words[((h >> np.uint64(18)) & np.uint64((1 << lw) - 1)).astype(np.int64)]
           >> ((h >> np.uint64(8)) & np.uint64(31)).astype(np.uint32)) & np.uint32(1)
    W = len(work) - n + 1
    if W <= 0:
        return 0
    ok = np.ones(W, dtype=bool)
    for j in range(n - K + 1):
        ok &= bit[j:j + W] == 1
    return int(ok.sum())
