"""Inputs of the long-script tests (test helper, no GPU): the script lengths at which the index
changes shape, and the small fan batches searched against them.

The script is synth.script_tokens(FULL) and its prefixes.  test_index_shape_host.py asserts on
the CPU that each prefix lies on the side of its edge that test_gpu_long_scripts.py expects, so
a change to `synth` fails there and not on the GPU.
"""

import collections
import functools

import numpy as np

from fandom_search_amd import synth
from fandom_search_amd.vocab import pack_strings

from tests import index_shape_restated as isr
from tests import levpairs, util

N = 6
EDGE = 1 << 18                                   # first script length without 8-byte records
FULL = EDGE + 64
RECORD_LENGTHS = (EDGE - 1, EDGE, EDGE + 1)
LSH_LENGTH = EDGE + 40
# prefix length -> G, its distinct 6-grams: either side of the two bucket-count edges
#   G / 4 <= 8192:  8 KB of seeds, which with the 32 KB filter fit a CU's LDS twice
#   G / 4 <= 16384: 16 KB of seeds, the most k_scan_rows keeps in LDS
EDGE_G = {32777: 32771, 32778: 32772, 65550: 65539, 65551: 65540}
TWO_PER_CU = (32777, 32778)
SEEDS_IN_LDS = (65550, 65551)
WORKS = [600] * 8
QUOTE = 40
LAST_AT, FIRST_AT = 100, 700                     # where the two quotes lie in the batch
RECORDS = 305                                    # of the oracle, at each of RECORD_LENGTHS
SATURATED_TOKENS = 12000                         # (the oracle searches one work on one thread: 0.55 ms a window)


@functools.lru_cache(maxsize=None)
def full_script():
    s = synth.script_tokens(FULL)
    s.setflags(write=False)
    return s


def script(length):
    return full_script()[:length]


@functools.lru_cache(maxsize=None)
def script_words(length):
    words = synth.vocab_words()
    return [words[t] for t in script(length).tolist()]


@functools.lru_cache(maxsize=None)
def grams(length):
    """G of a prefix, counted with numpy."""
    return isr.distinct_grams(script(length), N)


def plant(tok, scr):
    """The two quotes every case carries: the script's last and its first QUOTE tokens."""
    tok[LAST_AT:LAST_AT + QUOTE] = scr[len(scr) - QUOTE:]
    tok[FIRST_AT:FIRST_AT + QUOTE] = scr[:QUOTE]
    return tok


def corpus(length, extra=()):
    """Eight works of 600 tokens with the two quotes, and `extra` = ((position, tokens), ...)"""
    scr = script(length)
    tok, off = util.ragged_corpus(WORKS, scr)
    tok = plant(tok.copy(), scr)
    for at, ids in extra:
        tok[at:at + len(ids)] = ids
    return tok, off


def check_oracle_rows(want, length):
    """The conditions a case puts on the oracle's records before it compares the library's:
    both ends of the script are quoted, and every offset of the last script window occurs."""
    assert int(want["orig_ix"].max()) == length - 1
    assert int(want["orig_ix"].min()) == 0
    assert int((want["orig_ix"] >= length - N).sum()) == N
    assert sorted(want["orig_ix"][want["orig_ix"] >= length - N].tolist()) == list(range(length - N, length))


def high_bucket_window(length, log2_b=15, first_bucket=1 << 14, start=2000):
    """A script window that occurs once and whose n-gram falls into a bucket >= first_bucket of
    a table of 2^log2_b buckets: only a table with more than 2^14 buckets has such a bucket."""
    scr = script(length)
    h = isr.gram_hash(scr, N)
    b = isr.table_bucket(h, log2_b)
    grams = np.lib.stride_tricks.sliding_window_view(scr, N)
    for w in range(start, len(b)):
        if int(b[w]) >= first_bucket and int((grams == grams[w]).all(axis=1).sum()) == 1:
            return w, int(b[w])
    raise AssertionError("no such window")


HIGH_AT = 1300                                   # in the third work, away from the two quotes


@functools.lru_cache(maxsize=None)
def colliding_windows(length, count=3):
    """Pairs (a, b) of script windows that hold different n-grams with the same 32-bit hash.
    The slot of an n-gram is a function of its hash and its bucket's seed, so no seed separates
    the two: their bucket is one of those placed by linear probing (FS_DISP_OVERFLOW), and a
    lookup of either walks on from its slot."""
    scr = script(length)
    h = isr.gram_hash(scr, N)
    grams_ = np.lib.stride_tricks.sliding_window_view(scr, N)
    order = np.argsort(h, kind="stable")
    hs = h[order]
    out = []
    for i in np.nonzero(hs[1:] == hs[:-1])[0].tolist():
        a, b = int(order[i]), int(order[i + 1])
        if (grams_[a] != grams_[b]).any():
            out.append((a, b))
            if len(out) == count:
                break
    return tuple(out)


COLLIDING_AT = (1900, 2500, 3100)                # works 3, 4 and 5; the partner 50 tokens on


def colliding_corpus(length):
    """corpus(length) with both windows of each colliding pair quoted (one window each)."""
    scr = script(length)
    extra = []
    for at, (a, b) in zip(COLLIDING_AT, colliding_windows(length)):
        extra += [(at, scr[a:a + N]), (at + 50, scr[b:b + N])]
    tok, off = corpus(length, extra=tuple(extra))
    return tok, off, [at + d + k for at in COLLIDING_AT for d in (0, 50) for k in range(N)]


def saturated_batch(length):
    """One work of SATURATED_TOKENS tokens drawn like the script, from its vocabulary, with
    the two quotes and nothing else planted."""
    scr = script(length)
    tok = synth.script_tokens(SATURATED_TOKENS, seed=synth.SCRIPT_SEED + 1).copy()
    tok = plant(tok, scr)
    return tok, np.array([0, len(tok)], dtype=np.uint64)


FullRecord = collections.namedtuple(
    "FullRecord", "tok off tok_str chars coff lev fan_text script_text")


@functools.lru_cache(maxsize=None)
def full_record_batch(length=EDGE - 1):
    """The batch of corpus(length) with string ids of its own: the six fan tokens that quote the
    script's last window carry long strings, so that the record of the last of them holds
    orig_ix = length - 1 (bit 17, the top bit of its field, set), the window offset k = 5 (the
    largest) and a Levenshtein distance of 512..1023 (bit 9, the top bit of its field, set) at
    once: a field that runs into its neighbour shows.  `lev` is that distance by the plain DP."""
    words = synth.vocab_words()
    tok, off = corpus(length)
    rng = np.random.default_rng(18)
    _, fan = levpairs.content("disjoint", rng, 0, 600)
    fwords = levpairs.cut(fan, levpairs.split(600, N, "random", rng))
    tok_str = tok.copy()
    at = LAST_AT + QUOTE - N
    tok_str[at:at + N] = len(words) + np.arange(N, dtype=np.uint32)
    chars, coff = pack_strings(list(words) + fwords)
    stext = " ".join(words[t] for t in script(length)[length - N:].tolist())
    ftext = "[" + ", ".join(fwords) + "]"
    return FullRecord(tok, off, tok_str, chars, coff, levpairs.distance(stext, ftext), ftext, stext)
