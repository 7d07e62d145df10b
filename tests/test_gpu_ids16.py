"""k_scan_rows over the 16-bit copy of the fan ids (FS_SCAN_IDS16, DESIGN sections 5 and 6): two
pairs of sub-tiles in flight per wave, half the bytes per id.  The premixed ids are the same as
with the 32-bit stream, so every search here is run twice on ONE live index -- with the switch on
and with FS_SCAN_IDS16=0 -- and the two device buffers must be equal byte for byte, in all three
record forms (fs_row, 16-byte and 8-byte wire records), on one lane and on four.  Which stream a
search reads is asserted through the plan (fs_scan_shape.ids16), never through timing.  One small
corpus per window size is also held against the C oracle.

Shapes: the range count comes from fs_index_scan_shape (4096 on an MI355X); the corpora of the
range-length cases hold 0, 1, 2, 2.5, 3, 4 and 5 sub-tiles of 512 tokens per wave range on
average plus a rest that is no multiple of 512 -- shorter than the prefetch distance of two
pairs, both parities, and the tail that is read twice."""
import os

import numpy as np
import pytest

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings

from tests import util

pytestmark = pytest.mark.gpu

SWITCHES = ("FS_SCAN_IDS16", "FS_SCAN_ROWS", "FS_LANES", "FS_RANGES_CAPROW", "FS_ROWS_COOP", "FS_ROWS_XPOOL",
            "FS_DIAG", "FS_ROWS_FINISH", "FS_ROWS_SHARES", "FS_ROWS_WAVES", "FS_ROWS_BLOCKS_PER_CU")
FORMS = ((False, 32), (True, 16), (8, 8))          # fs_row, 16-byte and 8-byte wire records
DENSE_WORK, DENSE_LEN = 3, 1400


class _Env:
    """FS_* switches set for a block; with an index, its switches are read again on the way in
    and on the way out (fs_index_reload_switches: what tools/diag_ab.py does)."""

    def __init__(self, env, ix=None):
        self.env, self.ix = env, ix

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        os.environ.update(self.env)
        if self.ix is not None:
            self.ix.reload_switches()

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        if self.ix is not None:
            self.ix.reload_switches()


def _words(size):
    """`size` distinct lower-case pseudo-words of three syllables (synth.vocab_words ends at 10 000)."""
    syl = [c + v for c in "bcdfghjklmnprstvwxyz" for v in "aeiou"]
    return [syl[i // 10000] + syl[i // 100 % 100] + syl[i % 100] for i in range(size)]


def _setup(n, synth_base, script_len=5000):
    if n <= 6:
        words, emb, V = synth_base["words"], synth_base["emb"], synth.VOCAB_SIZE
        chars, coff = synth_base["chars"], synth_base["off"]
    else:                                          # (a one-hot table keeps n = 7, 8 on the exact path)
        V = 256
        words = synth.vocab_words(V)
        emb = np.eye(V, synth.EMB_DIM, dtype=np.float32)
        chars, coff = pack_strings(words)
    script = synth.script_tokens(script_len, vocab_size=V)
    return dict(n=n, V=V, words=words, emb=emb, chars=chars, coff=coff, script=script,
                swords=[words[int(t)] for t in script], normals=synth.lsh_normals(n),
                cfg=abi.make_config(window_size=n))


def _index(S, lanes):
    from fandom_search_amd.engine import ScriptIndex
    clear = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    try:
        with _Env({"FS_LANES": str(lanes)}):
            ix = ScriptIndex(S["script"], S["swords"], S["emb"], S["normals"], cfg=S["cfg"])
    finally:
        os.environ.update(clear)
    assert ix.info["path"] == abi.FS_MODE_EXACT
    return ix


def _corpus(n, V, script, first_work=0):
    """The small corpus: planted quotes as in test_gpu_rows_coop_lanes.py -- a dense stretch, a
    quote longer than one round, hits at work ends and across 512-token borders, empty and
    one-token works -- and a token count that is no multiple of 512."""
    lengths = [1500] * 40 + [0, 1, 5, n, n - 1, 3000, 511, 512, 513, 77]
    parts = [synth.fanwork_tokens(first_work + i, L, script, V) if L else np.zeros(0, np.uint32)
             for i, L in enumerate(lengths)]
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    tok = np.concatenate(parts).astype(np.uint32)
    assert len(tok) % 512 != 0
    d0 = int(off[DENSE_WORK])
    tok[d0:d0 + DENSE_LEN] = script[100 + first_work:100 + first_work + DENSE_LEN]   # dense: every window a hit
    tok[int(off[7]) + 1490:int(off[7]) + 1500] = script[40:50]  # hit at the end of a work ...
    tok[int(off[8]):int(off[8]) + 10] = script[40:50]           # ... and at the start of the next
    for k in range(9, 30):                                      # hits straddling 512-token borders
        at = (int(off[k]) // 512 + 1) * 512 - (k % (n + 3))
        tok[at:at + n + 2] = script[700 + k:700 + k + n + 2]
    for k, (ln, where) in enumerate(((90, 200), (150, 300), (300, 100), (150, 450))):   # one to five rounds each
        at = (int(off[31 + k]) // 512 + 1) * 512 + where
        tok[at:at + ln] = script[2000 + 400 * k:2000 + 400 * k + ln]
    return tok, off


def _device_bytes(ix, c, cap):
    """The device buffer of a search in each record form, as it lies there: the header's count
    and the records, unsorted."""
    import torch
    out = []
    for packed, size in FORMS:
        buf = torch.zeros(32 + cap * size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nw, _ = ix.search_end(ix.search_begin(c, buf.data_ptr(), cap, packed=packed, header=True))
        host = buf.cpu().numpy()
        assert int(host[:8].view(np.uint64)[0]) == nw
        out.append(host[:32 + nw * size].tobytes())
    return out


def _both_streams(ix, c, want16=True):
    """One corpus searched through both id streams of the live index `ix`: the plan says which
    one ran, the host rows and the device buffers of all forms are equal byte for byte.  Returns
    the rows."""
    assert ix.scan_shape(c)["waves"] > 0, "the search does not take k_scan_rows"
    assert ix.scan_ids16(c) == want16
    rows16, st16 = ix.search(c)
    dev16 = _device_bytes(ix, c, len(rows16) + 3)
    with _Env({"FS_SCAN_IDS16": "0"}, ix):
        assert ix.scan_shape(c)["waves"] > 0 and not ix.scan_ids16(c)
        rows32, st32 = ix.search(c)
        dev32 = _device_bytes(ix, c, len(rows32) + 3)
    assert ix.scan_ids16(c) == want16
    # (a corpus' first search may be repeated once with more staging room: DESIGN section 6)
    assert 1 <= st32.scan_launches <= st16.scan_launches <= 2
    assert rows16.tobytes() == rows32.tobytes()
    assert (st16.matches, st16.rows, st16.windows_processed) == (st32.matches, st32.rows, st32.windows_processed)
    for form, a, b in zip(FORMS, dev16, dev32):
        assert a == b, ("device buffer differs between the 16-bit and the 32-bit id stream", form)
    return rows16, st16


_SMALL = {}


def _small(n, synth_base):
    """Per n, once: the set-up, the small corpus and the oracle's rows."""
    if n not in _SMALL:
        S = _setup(n, synth_base)
        tok, off = _corpus(n, S["V"], S["script"])
        oi = util.oracle_index(S["cfg"], S["script"], S["words"], S["emb"], S["normals"])
        want, ost = oi.search(tok, off, S["chars"], S["coff"])
        oi.close()
        assert len(want) > DENSE_LEN
        _SMALL[n] = dict(S=S, tok=tok, off=off, want=want, want_matches=ost.matches)
    return _SMALL[n]


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7, 8])
def test_window_sizes_and_record_forms(synth_base, n, lanes):
    """n = 2..8, one lane and four, all record forms: both streams byte for byte, and the rows
    against the C oracle.  (130 sub-tiles over 4096 wave ranges: ranges of no and of one sub-tile.)"""
    ref = _small(n, synth_base)
    S = ref["S"]
    ix = _index(S, lanes)
    c = ix.corpus(ref["tok"], ref["off"], S["chars"], S["coff"])
    rows, st = _both_streams(ix, c)
    util.assert_rows_equal(rows, ref["want"])
    assert st.matches == ref["want_matches"]
    ix.close()


def _ranged_corpus(n, V, script, n_tok, seed):
    """n_tok tokens of uniform noise in works of 3000 (and a last shorter one), with a quote across
    every seventh 512-token border -- range borders among them -- at a varying offset, and a dense
    stretch and a long quote near the start."""
    rng = np.random.default_rng(seed)
    tok = rng.integers(0, V, size=n_tok, dtype=np.uint32)
    off = np.append(np.arange(0, n_tok, 3000, dtype=np.uint64), np.uint64(n_tok))
    for k, b in enumerate(range(512, n_tok - 600, 7 * 512)):
        at = b - (k % (n + 3))
        tok[at:at + n + 2] = script[700 + k % 2000:700 + k % 2000 + n + 2]
    if n_tok > 9000:
        tok[3100:3100 + 700] = script[100:800]
        tok[6500:6800] = script[2000:2300]
    return tok, off


@pytest.mark.parametrize("lanes", [1, 4])
def test_range_lengths(synth_base, lanes):
    """Sub-tiles per wave range: 0 (fewer sub-tiles than ranges), 1, 2, 3, 4, 5 and a mean of 2.5,
    each with 300 tokens over (a last sub-tile that is not full).  On one lane the sixteen waves of
    a workgroup take unequal shares of its sub-tiles, so each corpus holds ranges of several
    lengths around its mean; on four lanes the eight waves take equal ones."""
    n = 6
    S = _setup(n, synth_base)
    ix = _index(S, lanes)
    probe = ix.corpus(*_ranged_corpus(n, S["V"], S["script"], 20000, 1), S["chars"], S["coff"])
    shape = ix.scan_shape(probe)
    ranges = shape["waves"] * shape["blocks"]
    assert ranges >= 1024
    for i, per in enumerate((0.25, 1, 2, 2.5, 3, 4, 5)):
        n_tok = int(ranges * per) * 512 + 300
        tok, off = _ranged_corpus(n, S["V"], S["script"], n_tok, 10 + i)
        probe.update_begin(tok, off)
        probe.update_end()
        sh = ix.scan_shape(probe)
        assert sh["waves"] * sh["blocks"] == ranges
        rows, _ = _both_streams(ix, probe)
        assert len(rows) > 0
    ix.close()


_BIG = {}


def _big_table():
    """A table of 65 537 rows in synth.embedding's dimension (its first 65 536 rows are the table
    of exactly 2^16 rows), words for them, and a script that holds the ids 0, 65 535 and 65 536."""
    if not _BIG:
        V = 65537
        emb = synth.embedding(size=V, seed=synth.EMB_SEED + 1)
        words = _words(V)
        script = synth.script_tokens(1200, vocab_size=65536, seed=77)
        script[103], script[104] = 65535, 0           # both edge ids side by side inside one stretch
        script[300:306] = (0, 65535, 65535, 0, 0, 65535)
        script[500] = 65536                           # only the larger table has this row
        _BIG.update(V=V, emb=emb, words=words, script=script, strings=pack_strings(words))
    return _BIG


def _edge_corpus(script, V, n_tok=40 * 512 + 123, with_65536=False):
    rng = np.random.default_rng(5)
    tok = rng.integers(0, min(V, 65536), size=n_tok, dtype=np.uint32)
    off = np.append(np.arange(0, n_tok, 2500, dtype=np.uint64), np.uint64(n_tok))
    q = script[100:112]                               # q[3] = 65535, q[4] = 0
    for k, shift in enumerate((3, 4, 3 + 511, 4 + 511, 3 + 504, 4 + 7)):
        # id 65535 / id 0 as a sub-tile's first id (lane 0), its last id (lane 63) and the first
        # and last id of those lanes' eight
        at = 512 * (3 + 5 * k) - shift
        tok[at:at + 12] = q
    tok[512 * 33 - 2:512 * 33 + 4] = script[300:306]   # a window of edge ids only, across a border
    tok[0], tok[511], tok[512], tok[n_tok - 1] = 65535, 65535, 0, 65535   # and outside any quote
    if with_65536:
        tok[9000:9010] = script[495:505]
    return tok, off


@pytest.mark.parametrize("lanes", [1, 4])
def test_table_of_exactly_65536_rows(lanes):
    """Ids 0 and 65 535 inside quotes, at a sub-tile's first and last lane: the 16-bit stream runs
    and agrees with the 32-bit one."""
    B = _big_table()
    n, V = 6, 65536
    script = B["script"].copy()
    script[500] = 17
    words = B["words"][:V]
    S = dict(script=script, swords=[words[int(t)] for t in script], emb=B["emb"][:V],
             normals=synth.lsh_normals(n), cfg=abi.make_config(window_size=n))
    ix = _index(S, lanes)
    assert ix.info["path"] == abi.FS_MODE_EXACT
    chars, coff = pack_strings(words)
    tok, off = _edge_corpus(script, V)
    assert tok.max() == 65535 and tok.min() == 0
    c = ix.corpus(tok, off, chars, coff)
    rows, _ = _both_streams(ix, c, want16=True)
    hit = set(zip(rows["work"].tolist(), rows["fan_ix"].tolist()))
    for k, shift in enumerate((3, 4, 3 + 511, 4 + 511, 3 + 504, 4 + 7)):
        for p in (512 * (3 + 5 * k) - shift + 3, 512 * (3 + 5 * k) - shift + 4):   # the two edge ids of quote k
            w = int(np.searchsorted(off, p, side="right")) - 1
            assert (w, p - int(off[w])) in hit, (k, p)
    ix.close()


def test_table_of_65537_rows_takes_the_32_bit_stream():
    """Id 65 536 in the batch: no 16-bit copy, the search reads the 32-bit ids whatever the switch
    says and agrees with the chained kernels; a batch of the same table without such an id has the
    copy and uses it."""
    B = _big_table()
    n, V = 6, B["V"]
    S = dict(script=B["script"], swords=[B["words"][int(t)] for t in B["script"]], emb=B["emb"],
             normals=synth.lsh_normals(n), cfg=abi.make_config(window_size=n))
    ix = _index(S, 4)
    assert ix.info["path"] == abi.FS_MODE_EXACT
    chars, coff = B["strings"]
    tok, off = _edge_corpus(B["script"], V, with_65536=True)
    assert tok.max() == 65536
    c = ix.corpus(tok, off, chars, coff)
    rows, _ = _both_streams(ix, c, want16=False)
    with _Env({"FS_SCAN_ROWS": "0"}, ix):
        assert ix.scan_shape(c)["waves"] == 0
        chain, _ = ix.search(c)
    util.assert_rows_equal(rows, chain)
    w = int(np.searchsorted(off, 9005, side="right")) - 1
    assert (w, 9005 - int(off[w])) in set(zip(rows["work"].tolist(), rows["fan_ix"].tolist()))   # the id 65 536 itself
    tok2, off2 = _edge_corpus(B["script"], V)
    c.update_begin(tok2, off2)
    c.update_end()
    _both_streams(ix, c, want16=True)
    ix.close()


def test_updated_corpus_and_a_view_of_it(synth_base):
    """The copy is rebuilt with every upload (fs_corpus_update_begin/_end), and a view under a
    second script reads its base's copy."""
    n = 6
    ref = _small(n, synth_base)
    S = ref["S"]
    ix = _index(S, 4)
    c = ix.corpus(ref["tok"], ref["off"], S["chars"], S["coff"])
    rows, _ = _both_streams(ix, c)
    util.assert_rows_equal(rows, ref["want"])
    tok2, off2 = _corpus(n, S["V"], S["script"], first_work=100)
    tok2, off2 = tok2[:-37], off2.copy()
    off2[-1] -= 37
    c.update_begin(tok2, off2)
    c.update_end()
    rows2, _ = _both_streams(ix, c)
    assert len(rows2) > DENSE_LEN and rows2.tobytes() != rows.tobytes()
    with _Env({"FS_SCAN_ROWS": "0"}, ix):
        chain2, _ = ix.search(c)
    util.assert_rows_equal(rows2, chain2)
    # a second script (another stretch of the same source), its index, a view of the corpus
    S2 = dict(S)
    S2["script"] = np.concatenate([S["script"][1500:], S["script"][:1500]])
    S2["swords"] = [S["words"][int(t)] for t in S2["script"]]
    ix2 = _index(S2, 4)
    v = ix2.corpus_view(c)
    first, _ = ix2.search(v)                           # (a view's tables are built by its first search)
    vrows, _ = _both_streams(ix2, v)
    assert vrows.tobytes() == first.tobytes() and len(vrows) > DENSE_LEN
    c.update_begin(ref["tok"], ref["off"])             # a new batch of the base: the view follows
    c.update_end()
    vrows2, _ = _both_streams(ix2, v)
    own = ix2.corpus(ref["tok"], ref["off"], S["chars"], S["coff"])
    own_rows, _ = ix2.search(own)
    assert vrows2.tobytes() == own_rows.tobytes()
    ix2.close()
    ix.close()
