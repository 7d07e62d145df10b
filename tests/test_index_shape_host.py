"""The restated size rules of the script index (tests/index_shape_restated.py) against numbers
worked out by hand from the formulas, and the inputs of test_gpu_long_scripts.py: each script
prefix lies on the side of its edge that the GPU case expects.  No GPU."""

import numpy as np
import pytest

from fandom_search_amd import abi, synth

from tests import index_shape_restated as isr
from tests import levpairs, util
from tests import long_script_cases as lsc


# ---- the restatement against hand-worked numbers ------------------------------------------------

def test_record_form_edge():
    """18 bits of orig_ix: 2^18 - 1 tokens is the longest script with 8-byte records."""
    assert isr.host_wire8(262143) and not isr.host_wire8(262144) and not isr.host_wire8(262145)
    assert abi.PACKED8_MAX_SCRIPT == 262144 == lsc.EDGE
    # orig_ix | k << 18 | lev << 22 with every field full is a full word
    assert (262143 | 15 << 18 | 1023 << 22) == 0xFFFFFFFF


def test_lds_sizes_by_hand():
    # RangeLds 1152 + 512 + 256 + 512; FusedLds adds 768 + 256; CoopLds 3840 + 448 + 16 + 64
    assert isr.RANGE_LDS == 2432 and isr.FUSED_LDS == 3456 and isr.COOP_LDS == 4368
    # two workgroups of eight waves: 2 * (F + 1024 + 4368 + 8 * 3456) <= 163840  <=>  F <= 48880
    assert (isr.CU_LDS_BYTES // 2) - isr.COUNTERS_LDS - isr.COOP_LDS - 8 * isr.FUSED_LDS == 48880
    # one of sixteen: F <= 163840 - 1024 - 4368 - 55296 = 103152, which 64 KB + 16 KB always meet
    assert isr.CU_LDS_BYTES - isr.COUNTERS_LDS - isr.COOP_LDS - 16 * isr.FUSED_LDS == 103152


@pytest.mark.parametrize("G, lb, seeds", [
    (4, 2, 16), (32768, 13, 8192), (32771, 13, 8192), (32772, 14, 16384), (65536, 14, 16384),
    (65539, 14, 16384), (65540, 15, 0), (262144, 16, 0)])
def test_buckets_and_seeds(G, lb, seeds):
    """log2_buckets = ceil_log2(G / 4) (integer division): G = 32771 -> 8192 -> 13, G = 32772 ->
    8193 -> 14; G = 65539 -> 16384 -> 14, G = 65540 -> 16385 -> 15.  Seeds are bytes, in LDS up
    to 16 KB."""
    assert isr.log2_buckets(G) == lb
    assert isr.seeds_lds_bytes(G) == seeds
    assert isr.seeds_lds_bytes(G, disp_lds=False) == 0


@pytest.mark.parametrize("G, slots", [(7, 4), (32768, 17), (65540, 18), (131071, 18), (131072, 19),
                                      (262143, 19), (262144, 20)])
def test_slots(G, slots):
    """2G + 1 slots at least, so the table is at most half full: 2 * 131071 + 1 = 2^18 - 1 -> 18,
    2 * 131072 + 1 -> 19, 2 * 262143 + 1 = 2^19 - 1 -> 19, 2 * 262144 + 1 -> 20."""
    assert isr.log2_slots(G) == slots


@pytest.mark.parametrize("G, lw", [(100, 10), (1366, 10), (1367, 11), (21845, 14), (21846, 14),
                                   (21847, 15), (262144, 15)])
def test_bloom_filter_words(G, lw):
    """ceil_log2(3G / 4), 10..15: 3 * 21846 / 4 = 16384 -> 14, 3 * 21847 / 4 = 16385 -> 15;
    3 * 1366 / 4 = 1024 -> 10, 3 * 1367 / 4 = 1025 -> 11."""
    assert isr.bloom_log2_words(G) == lw


def test_sub_filter_words():
    """words = floor(S / (32 * 0.002^(1/3))) + 1, 32 * 0.002^(1/3) = 4.0317473...: 8192 words up
    to S = 33028 (33028 / 4.03175 = 8191.98), 8193 from 33029 (8192.23); 16384 up to 66056,
    16385 from 66057, which the clamp to 2^14 words holds down."""
    assert abs(32.0 * 2e-3 ** (1.0 / 3) - 4.0317473) < 1e-6
    assert isr.sub_k(6) == 4 and isr.sub_k(5) == 3 and isr.sub_k(3) == 0
    assert isr.sub_words_wanted(33028, 6) == 8192 and isr.sub_log2_words(33028, 6) == 13
    assert isr.sub_words_wanted(33029, 6) == 8193 and isr.sub_log2_words(33029, 6) == 14
    assert isr.sub_words_wanted(66056, 6) == 16384 and isr.sub_words_wanted(66057, 6) == 16385
    assert isr.sub_log2_words(66057, 6) == 14 == isr.sub_log2_words(1 << 18, 6)
    assert isr.sub_log2_words(100, 6) == 10
    # n = 5: K = 3, three tests per window as well
    assert isr.sub_words_wanted(33028, 5) == 8192


def test_launch_shape_rule():
    """32 KB of filter + 8 KB of seeds = 40960 <= 48880: twice on a CU; + 16 KB = 49152 misses by
    272 bytes.  One lane never takes the two-workgroup shape."""
    assert isr.rows_waves(32777, 32771, 6, lanes=4) == (8, 2)
    assert isr.rows_waves(32778, 32772, 6, lanes=4) == (16, 1)
    assert 32768 + 16384 - 48880 == 272
    assert isr.rows_waves(32777, 32771, 6, lanes=1) == (16, 1)
    # the 64 KB filter of a long script: never twice
    assert isr.rows_waves(1 << 18, 262000, 6, lanes=4) == (16, 1)
    assert isr.rows_fixed_lds(1 << 18, 262000, 6) == 65536 + 0 + 1024 + 4368


def test_hash_by_hand():
    """m(t) = (t mod 2^24) * 0x9E3779 mod 2^32; X = XOR rotl(m(t[k]), 7 (n - 1 - k));
    bucket = (h * 0x85EBCA6B mod 2^32) >> (32 - log2_buckets)."""
    assert int(isr.premix([1])[0]) == 0x9E3779
    assert int(isr.premix([0x1000002])[0]) == 2 * 0x9E3779          # (24 bits of the id)
    assert isr.gram_hash_one([1]) == 0x9E3779
    assert isr.gram_hash_one([1, 0]) == 0x4F1BBC80                    # 0x9E3779 << 7
    assert isr.gram_hash_one([0, 1]) == 0x9E3779
    assert isr.gram_hash_one([1, 1]) == 0x4F1BBC80 ^ 0x9E3779
    # 7 * 5 = 35 = 3 mod 32: the first of six ids is rotated by three
    assert isr.gram_hash_one([1, 0, 0, 0, 0, 0]) == 0x9E3779 << 3
    assert int(isr.table_bucket([1], 4)[0]) == 8                      # 0x85EBCA6B >> 28
    assert int(isr.table_bucket([2], 15)[0]) == (0x0BD794D6 >> 17)    # 2 * 0x85EBCA6B mod 2^32
    # K = 4: P = m0 << 24 + m1 << 16 + m2 << 8 + m3 mod 2^32
    assert int(isr.sub_hash([1, 0, 0, 1], 4)[0]) == ((0x9E3779 << 24) + 0x9E3779) & 0xFFFFFFFF


def test_vector_and_scalar_hash_agree():
    scr = lsc.script(5000)
    h = isr.gram_hash(scr, 6)
    for w in (0, 1, 777, 4994):
        assert int(h[w]) == isr.gram_hash_one(scr[w:w + 6])
    assert len(h) == 4995


# ---- the inputs of the GPU cases ----------------------------------------------------------------

def test_script_is_a_prefix_family():
    assert lsc.full_script().tolist()[:3000] == synth.script_tokens(3000).tolist()
    assert len(lsc.full_script()) == (1 << 18) + 64


@pytest.mark.parametrize("length", sorted(lsc.EDGE_G))
def test_prefixes_sit_at_the_bucket_edges(length):
    G = isr.distinct_grams(lsc.script(length), 6)
    assert G == lsc.EDGE_G[length]


def test_edge_prefixes_take_the_expected_sides():
    lo, hi = lsc.TWO_PER_CU
    assert isr.rows_waves(lo, lsc.EDGE_G[lo], 6, 4) == (8, 2) and isr.rows_waves(hi, lsc.EDGE_G[hi], 6, 4) == (16, 1)
    assert isr.sub_log2_words(lo, 6) == isr.sub_log2_words(hi, 6) == 13      # the seeds alone flip the shape
    lo, hi = lsc.SEEDS_IN_LDS
    assert isr.seeds_lds_bytes(lsc.EDGE_G[lo]) == 16384 and isr.log2_buckets(lsc.EDGE_G[lo]) == 14
    assert isr.seeds_lds_bytes(lsc.EDGE_G[hi]) == 0 and isr.log2_buckets(lsc.EDGE_G[hi]) == 15
    assert isr.sub_log2_words(lo, 6) == 14


def test_high_bucket_window():
    """The quote planted for the seeds-in-memory case: a script window that occurs once, in a
    bucket that only a table of more than 2^14 buckets has."""
    hi = lsc.SEEDS_IN_LDS[1]
    w, b = lsc.high_bucket_window(hi)
    scr = lsc.script(hi)
    assert b >= 16384 and b == (isr.gram_hash_one(scr[w:w + 6]) * 0x85EBCA6B & 0xFFFFFFFF) >> 17
    assert w + 12 <= lsc.SEEDS_IN_LDS[0]                  # the same quote exists in the shorter prefix


def test_colliding_windows():
    """The quotes planted for the overflow-bucket case: different n-grams, one hash."""
    scr = lsc.script(lsc.EDGE)
    pairs = lsc.colliding_windows(lsc.EDGE)
    assert len(pairs) == 3
    for a, b in pairs:
        assert scr[a:a + 6].tolist() != scr[b:b + 6].tolist()
        assert isr.gram_hash_one(scr[a:a + 6]) == isr.gram_hash_one(scr[b:b + 6])
    tok, off, planted = lsc.colliding_corpus(lsc.EDGE)
    assert len(planted) == 36 and tok[1950:1956].tolist() == scr[pairs[0][1]:pairs[0][1] + 6].tolist()


@pytest.fixture(scope="module")
def base():
    from fandom_search_amd.vocab import pack_strings
    words = synth.vocab_words()
    chars, off = pack_strings(words)
    return dict(words=words, emb=synth.embedding(), chars=chars, off=off, normals=synth.lsh_normals(6))


def test_full_record_batch_on_the_oracle(base):
    """2^18 - 1 tokens: the oracle's records reach both ends of the script, all six offsets of
    the last window occur, and the record of the last script word holds a Levenshtein distance of
    512..1023, the plain DP's, while orig_ix and k are at their largest."""
    L = lsc.EDGE - 1
    fr = lsc.full_record_batch(L)
    assert 512 <= fr.lev <= 1023
    assert fr.lev == levpairs.distance_plain(fr.script_text, fr.fan_text)
    oi = util.oracle_index(abi.make_config(), lsc.script(L), base["words"], base["emb"], base["normals"],
                           swords=lsc.script_words(L))
    want, _ = oi.search(fr.tok, fr.off, fr.chars, fr.coff, tok_str=fr.tok_str)
    oi.close()
    lsc.check_oracle_rows(want, L)
    assert len(want) == lsc.RECORDS
    full = want[(want["orig_ix"] == L - 1)]
    assert len(full) == 1 and int(full["orig_ix"][0]) >= lsc.EDGE - 7
    assert int(full["lev"][0]) == fr.lev
    assert int(full["fan_ix"][0]) == lsc.LAST_AT + lsc.QUOTE - 1 and int(full["work"][0]) == 0


def test_saturated_filter_batch(base):
    """2^18 + 1 tokens: the sub-shingle filter is 2^14 words whatever the script's length from
    66,057 tokens on, its bit density here about 0.4, so about 0.4^3 = 6 % of all windows pass.
    The windows it lets through outnumber the windows that match by more than ten to one.
    (`matches` counts (window, script window) pairs: with the default configuration, nearest_n =
    10 and no UniqueFilter, each matching window counts ten, so candidates against matches is
    about two to one; the load of the rounds is counted in windows.)"""
    L = lsc.EDGE + 1
    scr = lsc.script(L)
    dens = isr.sub_filter_density(isr.sub_filter(scr, 6))
    assert 0.3 < dens < 0.5, dens
    tok, off = lsc.saturated_batch(L)
    passed = isr.sub_pass_count(tok, scr, 6)
    true = isr.matching_windows(tok, scr, 6)
    cfg = abi.make_config()
    oi = util.oracle_index(cfg, scr, base["words"], base["emb"], base["normals"], swords=lsc.script_words(L))
    want, st = oi.search(tok, off, base["chars"], base["off"])
    oi.close()
    lsc.check_oracle_rows(want, L)
    print("density %.3f, windows passed %d, windows that match %d, oracle matches %d, records %d"
          % (dens, passed, true, st.matches, len(want)))
    assert st.matches == cfg.nearest_n * true
    assert passed > 10 * true
