"""Verification out of the 16-bit copy of the fan ids (fs_ranges.h range_round<N, STR, I16>; DESIGN
section 6): on a batch that has the copy k_scan_rows takes a candidate's ids from the aligned
dwords of tok16 instead of the 32-bit array.  Every search here runs on ONE live index with the
16-bit stream and with FS_SCAN_IDS16=0 (test_gpu_ids16._both_streams): host rows and the device
buffers of the three record forms must be equal byte for byte, on one lane and on four.  The cases
aim at what the existing suites do not: candidates and halo windows at both parities around
sub-tile and range borders, the two ends of the buffer, the ids 0 and 65 535 side by side, and
windows that differ from a script n-gram in one slot and still pass the filter.  One corpus per
window size is also held against the C oracle.  Nothing here reads a time, a counter or assembly."""
import numpy as np
import pytest

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings

from tests import util
from tests.test_gpu_ids16 import _Env, _big_table, _both_streams, _edge_corpus, _index, _setup

pytestmark = pytest.mark.gpu

SIZES = (2, 3, 4, 5, 6, 7, 8)
SMALL_TOK = 40 * 512


def _streams(ix, c):
    """_both_streams, and the candidate count, which must not depend on the stream either."""
    rows, st16 = _both_streams(ix, c)
    with _Env({"FS_SCAN_IDS16": "0"}, ix):
        _, st32 = ix.search(c)
    assert st16.candidates == st32.candidates
    return rows, st32


def _chained(ix, c):
    with _Env({"FS_SCAN_ROWS": "0"}, ix):
        assert ix.scan_shape(c)["waves"] == 0
        rows, _ = ix.search(c)
    return rows


# ---- candidate parity and borders ---------------------------------------------------

def _border_corpus(n, V, script, n_tok, seed):
    """Uniform noise in works of 3000 tokens; ONE quote of n + 4 tokens (five windows, both
    parities) planted around every seventh 512-token border at the offsets -8 .. +8 in turn: it
    ends in front of the border, straddles it at every alignment or starts on and behind it, so
    candidates fall on a sub-tile's last and first lane and the windows in front of a range start
    (verified whatever the filter says) are quote and noise at both parities."""
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, V, size=n_tok, dtype=np.uint32)
    off = np.append(np.arange(0, n_tok, 3000, dtype=np.uint64), np.uint64(n_tok))
    quote = script[700:700 + n + 4]
    for k, b in enumerate(range(512, n_tok - 600, 7 * 512)):
        at = b + (k % 17) - 8
        tok[at:at + len(quote)] = quote
    return tok, off


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", SIZES)
def test_candidate_parity_around_borders(synth_base, n, lanes):
    """Mean range lengths of 1 and 2.5 sub-tiles over the launch's 4096 wave ranges: where the
    prefetch distance of two pairs and the range end meet."""
    S = _setup(n, synth_base)
    ix = _index(S, lanes)
    c = ix.corpus(*_border_corpus(n, S["V"], S["script"], 20000, 1), S["chars"], S["coff"])
    shape = ix.scan_shape(c)
    ranges = shape["waves"] * shape["blocks"]
    assert ranges >= 1024
    for i, per in enumerate((1, 2.5)):
        n_tok = int(ranges * per) * 512 + 300
        tok, off = _border_corpus(n, S["V"], S["script"], n_tok, 20 + i)
        c.update_begin(tok, off)
        c.update_end()
        sh = ix.scan_shape(c)
        assert sh["waves"] * sh["blocks"] == ranges
        rows, _ = _streams(ix, c)
        # every planted quote is found: its n + 4 words, wherever the border cuts it
        found = np.zeros(n_tok, dtype=bool)
        found[off[rows["work"]].astype(np.int64) + rows["fan_ix"]] = True
        for k, b in enumerate(range(512, n_tok - 600, 7 * 512)):
            at = b + (k % 17) - 8
            cut = [int(x) for x in off if at < x < at + n + 4]          # a work border inside the quote
            if not cut:
                assert found[at:at + n + 4].all(), (per, k, at)
    ix.close()


# ---- the ends of the buffer ------------------------------------------------------------

def _end_corpora(n, V, script):
    """Four batches of about 40 x 512 tokens: (even, odd token count) x (long works, works of n - 1,
    n and n + 1 tokens at both ends).  Long works: a quote at p = 0 (even count) or p = 1 (odd
    count) and one whose last window ends exactly at the last token.  Short works: each holds a
    script stretch, so the windows inside a work of n or n + 1 tokens are hits and the candidates
    that cross into the neighbour are turned down by the work's end."""
    out = []
    for odd in (0, 1):
        n_tok = SMALL_TOK + 122 + odd
        rng = np.random.default_rng(40 + odd)
        tok = rng.integers(0, V, size=n_tok, dtype=np.uint32)
        off = np.append(np.arange(0, n_tok, 2500, dtype=np.uint64), np.uint64(n_tok))
        tok[odd:odd + n + 3] = script[50:50 + n + 3]
        tok[n_tok - n - 3:] = script[90:90 + n + 3]
        tok[5 * 512 - 3:5 * 512 + n + 2] = script[130:130 + n + 5]
        out.append((tok.copy(), off))
        ends = [n - 1, n, n + 1]
        lens = ends + [2500] * 7 + [n_tok - 2 * sum(ends) - 7 * 2500] + ends[::-1]
        off2 = np.zeros(len(lens) + 1, dtype=np.uint64)
        off2[1:] = np.cumsum(lens)
        assert int(off2[-1]) == n_tok
        tok2 = tok.copy()
        tok2[:sum(ends)] = script[200:200 + sum(ends)]
        tok2[n_tok - sum(ends):] = script[300:300 + sum(ends)]
        out.append((tok2, off2))
    assert sorted(len(t) % 2 for t, _ in out) == [0, 0, 1, 1]
    return out


_ENDS = {}


def _ends(n, synth_base):
    """Per n, once: the set-up, the four batches and the oracle's rows of each."""
    if n not in _ENDS:
        S = _setup(n, synth_base, script_len=1200)
        batches = _end_corpora(n, S["V"], S["script"])
        oi = util.oracle_index(S["cfg"], S["script"], S["words"], S["emb"], S["normals"])
        want = [oi.search(tok, off, S["chars"], S["coff"])[0] for tok, off in batches]
        oi.close()
        _ENDS[n] = dict(S=S, batches=batches, want=want)
    return _ENDS[n]


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", SIZES)
def test_ends_of_the_buffer(synth_base, n, lanes):
    ref = _ends(n, synth_base)
    S = ref["S"]
    ix = _index(S, lanes)
    c = None
    for (tok, off), want in zip(ref["batches"], ref["want"]):
        if c is None:
            c = ix.corpus(tok, off, S["chars"], S["coff"])
        else:
            c.update_begin(tok, off)
            c.update_end()
        rows, _ = _streams(ix, c)
        util.assert_rows_equal(rows, want)
        n_tok = len(tok)
        hit = set((off[rows["work"]].astype(np.int64) + rows["fan_ix"]).tolist())
        if len(off) < 12:                                # long works: the quote at p = 0 / p = 1 ...
            assert n_tok % 2 in hit and (n_tok % 2 == 0 or 0 not in hit)
            assert n_tok - 1 in hit                      # ... and the window that ends at the last token
        else:                                            # works of n - 1, n, n + 1 tokens at both ends
            assert 0 not in hit and n - 1 in hit and 2 * n - 1 in hit
            assert n_tok - 1 not in hit and n_tok - n + 1 not in hit and n_tok - n in hit
    ix.close()


# ---- the ids 0 and 65 535, and near misses: a table of exactly 65 536 rows ---------------

def _big_setup(n):
    """The 65 536-row table of test_gpu_ids16 and its script (ids over the whole 16 bits).  For
    n = 7, 8 the exact path's proof needs more room than the default threshold leaves with this
    table (cos bound (n - 1 + c_max) / n): a threshold of 0.01 keeps those indexes exact -- the
    exact path reports id-identical windows only, so what the searches find does not change."""
    B = _big_table()
    V = 65536
    script = B["script"].copy()
    script[500] = 17
    words = B["words"][:V]
    cfg = abi.make_config(window_size=n, distance_threshold=0.1 if n <= 6 else 0.01)
    return dict(n=n, V=V, script=script, words=words, swords=[words[int(t)] for t in script],
                emb=B["emb"][:V], normals=synth.lsh_normals(n), cfg=cfg)


_BIG_STRINGS = []


def _big_strings():
    if not _BIG_STRINGS:
        _BIG_STRINGS.extend(pack_strings(_big_table()["words"][:65536]))
    return _BIG_STRINGS


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", [2, 5, 6])
def test_edge_ids_side_by_side(n, lanes):
    """script[300:306] = (0, 65535, 65535, 0, 0, 65535): both orders of the two edge ids.  The
    stretch around it is planted at even and odd positions, inside a sub-tile and across borders."""
    S = _big_setup(n)
    ix = _index(S, lanes)
    chars, coff = _big_strings()
    tok, off = _edge_corpus(S["script"], S["V"])
    stretch = S["script"][296:310]
    starts = [1000, 1031, 512 * 9 - 7, 512 * 14 - 8, 512 * 21 - 4, 512 * 26 - 5, 512 * 30 + 0, 512 * 36 + 1]
    assert sorted(s % 2 for s in starts) == [0] * 4 + [1] * 4
    for at in starts:
        tok[at:at + len(stretch)] = stretch
    assert tok.max() == 65535 and tok.min() == 0
    c = ix.corpus(tok, off, chars, coff)
    rows, _ = _streams(ix, c)
    util.assert_rows_equal(rows, _chained(ix, c))
    hit = set((off[rows["work"]].astype(np.int64) + rows["fan_ix"]).tolist())
    for at in starts:
        if not any(at < int(x) < at + len(stretch) for x in off):
            assert all(p in hit for p in range(at, at + len(stretch))), at
    ix.close()


KINDS = ("bit 0 flipped", "bit 15 flipped", "bytes swapped", "the neighbouring slot's id")
# noise seeds per n, fixed on an MI355X with the 32-bit stream (the reference of this test): with
# them the filter lets at least 16 windows through that are no script n-gram (asserted below;
# seed 1, n = 2 .. 8: 63, 84, 286, 221, 292, 231 and 226 such windows, on one lane and on four)
NEAR_SEED = {2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1}


def _near_corpus(n, script, seed):
    """About two thousand windows that equal a script n-gram except in one slot -- each slot
    0 .. n - 1, each of the four replacements, both parities of the position -- packed n + 3 apart
    into noise."""
    n_tok = 44 * 512 + 77
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, 65536, size=n_tok, dtype=np.uint32)
    off = np.append(np.arange(0, n_tok, 2500, dtype=np.uint64), np.uint64(n_tok))
    stride = n + 3
    count = min(2000, (n_tok - 16) // stride)
    seen = set()
    for i in range(count):
        slot, kind, odd = i % n, (i // n) % 4, (i // (4 * n)) % 2
        s = (i * 7) % (len(script) - n)
        w = script[s:s + n].astype(np.uint32).copy()
        v = int(w[slot])
        w[slot] = (v ^ 1, v ^ 0x8000, ((v & 0xFF) << 8) | (v >> 8), int(w[slot + 1 if slot + 1 < n else slot - 1]))[kind]
        at = 8 + i * stride + odd
        tok[at:at + n] = w
        seen.add((slot, kind, at % 2))
    assert len(seen) == n * 4 * 2
    return tok, off, count


def _script_ngram_windows(tok, script, n):
    """Fan windows (anywhere in the buffer) whose ids equal a script n-gram's."""
    view = np.lib.stride_tricks.sliding_window_view
    grams = set(w.tobytes() for w in view(script.astype(np.uint32), n))
    return sum(1 for w in view(tok.astype(np.uint32), n) if w.tobytes() in grams)


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", SIZES)
def test_near_misses_reach_verification_and_are_turned_down(n, lanes):
    """The id compare of verification is what rejects these windows, and it reads the ids from the
    16-bit copy: a half-word taken from the wrong dword, a shift by one id or a lost top bit would
    turn a near miss into a hit or a hit into a miss."""
    S = _big_setup(n)
    ix = _index(S, lanes)
    chars, coff = _big_strings()
    tok, off, count = _near_corpus(n, S["script"], NEAR_SEED[n])
    assert count >= 1800
    # a few whole quotes among them, so that hits and near misses share rounds
    for k, at in enumerate(range(8 + count * (n + 3) + 4, len(tok) - 2 * n - 8, 97)):
        s = 40 + 9 * k % 1000
        tok[at + k % 2:at + k % 2 + n + 2] = S["script"][s:s + n + 2]
    c = ix.corpus(tok, off, chars, coff)
    rows, st32 = _streams(ix, c)
    equal = _script_ngram_windows(tok, S["script"], n)
    print("n %d lanes %d: candidates %d, windows equal to a script n-gram %d, turned down %d"
          % (n, lanes, st32.candidates, equal, st32.candidates - equal))
    assert equal > 0 and len(rows) > 0
    assert st32.candidates >= equal + 16, "too few windows reach verification only to be turned down"
    util.assert_rows_equal(rows, _chained(ix, c))
    ix.close()
