"""The search at the script lengths where the index changes shape.

The index build and the launch choose buffer sizes, kernel instances, launch shapes and the
record format by the script's length (tests/index_shape_restated.py has the rules).  Every case
here sits on one side of such an edge, says so through ScriptIndex.scan_shape (a case that stops
reaching its branch fails), and is compared bit for bit with the C oracle.  The fan batches are
small (tests/long_script_cases.py): eight works of 600 tokens that quote the script's first and
last 40 tokens, so that script positions 0 and n_script - 1 and every offset of the last script
window occur in the records.  test_index_shape_host.py holds the inputs on their sides of the
edges without a GPU.
"""

import os

import numpy as np
import pytest

from fandom_search_amd import abi, synth

from tests import index_shape_restated as isr
from tests import long_script_cases as lsc
from tests import util

pytestmark = pytest.mark.gpu

SWITCHES = ("FS_SCAN_ROWS", "FS_RANGES_CAPROW", "FS_LANES", "FS_ROWS_DISP_LDS", "FS_ROWS_COOP",
            "FS_ROWS_XPOOL", "FS_DIAG", "FS_ROWS_FINISH", "FS_ROWS_SHARES", "FS_FILTER_LOG2_WORDS",
            "FS_SFILTER_LOG2_WORDS", "FS_SCAN_SUB", "FS_HOST_WIRE8", "FS_ROWS_WAVES",
            "FS_ROWS_BLOCKS_PER_CU")
VARIANTS = {"one_lane": {}, "lanes4": {"FS_LANES": "4"}, "chain": {"FS_SCAN_ROWS": "0"}}
N = lsc.N


class _Env:
    """The FS_* switches of one index, set while it is created (they are read there)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def base(synth_base):
    return dict(synth_base, normals=synth.lsh_normals(N))


@pytest.fixture(scope="module")
def oracle(base):
    """oracle(length) -> the C oracle's index of that script prefix, one per length for the
    whole module; oracle.rows(length, key, search) keeps a batch's records."""
    made, kept = {}, {}

    def get(length):
        if length not in made:
            made[length] = util.oracle_index(abi.make_config(), lsc.script(length), base["words"], base["emb"],
                                             base["normals"], threads=8, swords=lsc.script_words(length))
        return made[length]

    def rows(length, key, tok, off, chars, coff, tok_str=None):
        if (length, key) not in kept:
            want, st = get(length).search(tok, off, chars, coff, tok_str=tok_str)
            want.setflags(write=False)
            kept[(length, key)] = (want, st)
        return kept[(length, key)]
    get.rows = rows
    yield get
    for oi in made.values():
        oi.close()


def _index(base, length, env, **cfg_kw):
    from fandom_search_amd.engine import ScriptIndex
    with _Env(env):
        ix = ScriptIndex(lsc.script(length), lsc.script_words(length), base["emb"], base["normals"],
                         cfg=abi.make_config(**cfg_kw))
    assert ix.info["n_script"] == length and ix.info["n_grams"] == lsc.grams(length)
    return ix


def _shape(ix, c, label):
    shape = ix.scan_shape(c)
    print("scan_shape %s: %s" % (label, shape))
    length, G = int(ix.info["n_script"]), int(ix.info["n_grams"])
    # what does not depend on the switches: the table's geometry and the host record form
    assert shape["log2_buckets"] == isr.log2_buckets(G)
    assert shape["log2_slots"] == isr.log2_slots(G)
    assert shape["host_wire8"] == int(isr.host_wire8(length) and ix.info["path"] == abi.FS_MODE_EXACT)
    # (issue: a bucket whose seed is no byte needs a planted hit of its own)
    assert shape["wide_buckets"] == 0
    return shape


def _device_rows(ix, c, n_want, off, eight):
    """fs_row records of a device search in each record form: as they are, from 16-byte wire
    records through unpack_device, and from 8-byte ones through unpack8_device -- or, with
    `eight` false, the refusal of both 8-byte calls."""
    import torch
    from fandom_search_amd import _lib
    cap = n_want + 8
    rows = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    p16 = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
    p8 = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    full = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()          # torch's fills are complete before the library's streams write
    out = {}
    n, _ = ix.search_device(c, rows.data_ptr(), cap)
    out["fs_row"] = rows.cpu().numpy()[:n * 32].view(abi.ROW_DTYPE)
    n, _ = ix.search_device(c, p16.data_ptr(), cap, packed=True)
    ix.unpack_device(p16.data_ptr(), n, full.data_ptr())
    out["16 bytes"] = full.cpu().numpy()[:n * 32].view(abi.ROW_DTYPE).copy()
    if eight:
        n, _ = ix.search_device(c, p8.data_ptr(), cap, packed=8)
        full.zero_()
        torch.cuda.synchronize()
        ix.unpack8_device(p8.data_ptr(), n, d_off.data_ptr(), len(off) - 1, full.data_ptr())
        out["8 bytes"] = full.cpu().numpy()[:n * 32].view(abi.ROW_DTYPE).copy()
    else:
        with pytest.raises(_lib.FsError) as e:
            ix.search_device(c, p8.data_ptr(), cap, packed=8)
        assert e.value.code == abi.FS_E_UNSUPPORTED
        with pytest.raises(_lib.FsError) as e:
            ix.unpack8_device(p8.data_ptr(), 1, d_off.data_ptr(), len(off) - 1, full.data_ptr())
        assert e.value.code == abi.FS_E_UNSUPPORTED
    return out


def _check_search(ix, c, want, ost, off, eight):
    got, st = ix.search(c)
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
    for form, rows in _device_rows(ix, c, len(want), off, eight).items():
        assert rows.tobytes() == want.tobytes(), form
    return st


# ---- the record form: 2^18 - 1, 2^18, 2^18 + 1 tokens -------------------------------------------

@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("length", lsc.RECORD_LENGTHS)
def test_record_form_at_the_edge(base, oracle, length, variant):
    """Below 2^18 script tokens a host search and fs_rows_unpack8 carry 8-byte records
    {token position, orig_ix | k << 18 | lev << 22}; from 2^18 on the 16-byte form, and the
    8-byte calls are FS_E_UNSUPPORTED.  Host search, fs_row, 16-byte and 8-byte device searches
    against the oracle, whose records hold orig_ix = 0, orig_ix = n_script - 1 and all six
    offsets of the last script window: an orig_ix that ran into the bits of k would come back as
    another script position with another distance.  One lane, four lanes (the k_scan_rows
    instance that ends in k_compact) and the chained kernels; every long script runs the
    2^14-word (LW14) filter instance with its seeds read from memory."""
    tok, off = lsc.corpus(length)
    want, ost = oracle.rows(length, "plain", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, length)
    assert len(want) == lsc.RECORDS
    ix = _index(base, length, VARIANTS[variant])
    assert ix.info["path"] == abi.FS_MODE_EXACT
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d %s" % (length, variant))
    eight = length < lsc.EDGE
    assert shape["host_wire8"] == int(eight)
    if variant == "chain":
        assert shape["waves"] == 0 and shape["blocks"] == 0
        assert shape["filter_log2_words"] == 15 == isr.bloom_log2_words(lsc.grams(length))
    else:
        assert shape["waves"] == 16 and shape["blocks"] > 0
        assert shape["filter_log2_words"] == 14 and shape["seeds_lds_bytes"] == 0
    assert shape["log2_slots"] == 19 and shape["log2_buckets"] == 16
    _check_search(ix, c, want, ost, off, eight)
    ix.close()


@pytest.mark.parametrize("length", lsc.RECORD_LENGTHS)
def test_python_layer_picks_its_record_form(base, oracle, tmp_path, length):
    """AnnIndexSearch over the same works as files: search_batch (a host search) and the sharded
    search, which leaves wire records on the device and picks their form from
    abi.PACKED8_MAX_SCRIPT.  Both must give the oracle's records."""
    from fandom_search_amd import dist, search, vocab
    words = base["words"]
    tok, off = lsc.corpus(length)
    want, _ = oracle.rows(length, "plain", tok, off, base["chars"], base["off"])
    (tmp_path / "script.txt").write_text(synth.script_markup(lsc.script(length), words))
    files = []
    for w in range(len(off) - 1):
        files.append(str(tmp_path / synth.work_name(w)))
        with open(files[-1], "w", encoding="utf8") as fh:
            fh.write(" ".join(words[t] for t in tok[int(off[w]):int(off[w + 1])].tolist()))
    ann = search.AnnIndexSearch(str(tmp_path / "script.txt"), N, 15, 14, 0.1, vocab=vocab.Vocab(words, base["emb"]),
                                normals=base["normals"])
    assert len(ann.word_lowercase) == length and ann.engine.info["path"] == abi.FS_MODE_EXACT
    recs = ann.search_batch(files)
    assert len(recs) == len(want)
    got = np.array([(files.index(r[0]), r[1], r[4], r[10], r[9], r[11]) for r in recs], dtype=abi.ROW_DTYPE)
    util.assert_rows_equal(got, want)
    assert [r[5] for r in recs] == [words[t] for t in lsc.script(length)[want["orig_ix"]].tolist()]
    rows, fan_words = dist.search_sharded(files, [1] * len(files), ann)
    util.assert_rows_equal(rows, want)
    pos = off[want["work"]].astype(np.int64) + want["fan_ix"].astype(np.int64)
    assert fan_words == [words[t] for t in tok[pos].tolist()]
    ann.engine.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_eight_byte_record_with_every_field_full(base, oracle, variant):
    """2^18 - 1 tokens, string ids of the batch's own: the fan tokens that quote the last script
    window carry long strings, so the oracle's record of the last script word holds orig_ix =
    2^18 - 2 (>= 2^18 - 7, bit 17 set), window offset k = 5 and a Levenshtein distance of
    512..1023 (bit 9 set; the plain DP's, test_index_shape_host.py) in one 8-byte record: a field
    that bleeds into its neighbour shows."""
    L = lsc.EDGE - 1
    fr = lsc.full_record_batch(L)
    want, ost = oracle.rows(L, "full", fr.tok, fr.off, fr.chars, fr.coff, tok_str=fr.tok_str)
    lsc.check_oracle_rows(want, L)
    full = want[want["orig_ix"] == L - 1]           # (only offset 5 of the last window reaches the last word)
    assert len(full) == 1 and int(full["orig_ix"][0]) >= lsc.EDGE - 7
    assert 512 <= int(full["lev"][0]) <= 1023 and int(full["lev"][0]) == fr.lev
    ix = _index(base, L, VARIANTS[variant])
    c = ix.corpus(fr.tok, fr.off, fr.chars, fr.coff, tok_str=fr.tok_str)
    shape = _shape(ix, c, "%d %s, string ids" % (L, variant))
    assert shape["host_wire8"] == 1
    assert (shape["waves"] == 0) == (variant == "chain")
    _check_search(ix, c, want, ost, fr.off, True)
    ix.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_hits_in_overflow_buckets(base, oracle, variant):
    """A script of 2^18 tokens holds some dozens of pairs of different 6-grams with one 32-bit
    hash (27 by the restated hash, 25 overflow buckets); no seed separates such a pair, its
    bucket is placed by linear probing and a lookup walks on from its slot.  The batch quotes
    both windows of three pairs; the oracle has records at every quoted token."""
    L = lsc.EDGE
    tok, off, planted = lsc.colliding_corpus(L)
    want, ost = oracle.rows(L, "colliding", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, L)
    pos = set((off[want["work"]].astype(np.int64) + want["fan_ix"].astype(np.int64)).tolist())
    assert pos.issuperset(planted)
    ix = _index(base, L, VARIANTS[variant])
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d %s, colliding hashes" % (L, variant))
    assert shape["overflow_buckets"] >= 1
    _check_search(ix, c, want, ost, off, False)
    ix.close()


# ---- the seeds of the exact table: in LDS up to 2^14 buckets ------------------------------------

@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("length", lsc.SEEDS_IN_LDS)
def test_seeds_in_lds_or_in_memory(base, oracle, length, lanes):
    """G = 65,539 distinct 6-grams: 2^14 buckets, 16 KB of seeds in LDS; G = 65,540: 2^15
    buckets, read from memory.  The batch also quotes a script window whose n-gram lies, by the
    restated hash, in a bucket >= 2^14 of the larger table -- a bucket the smaller one lacks."""
    w, bucket = lsc.high_bucket_window(lsc.SEEDS_IN_LDS[1])
    tok, off = lsc.corpus(length, extra=((lsc.HIGH_AT, lsc.script(length)[w:w + 2 * N]),))
    want, ost = oracle.rows(length, "high", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, length)
    assert bucket >= 1 << 14 and (want["orig_ix"] == w).any()
    ix = _index(base, length, {"FS_LANES": str(lanes)})
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d lanes %d" % (length, lanes))
    assert shape["waves"] == 16 and shape["filter_log2_words"] == 14
    if length == lsc.SEEDS_IN_LDS[0]:
        assert shape["seeds_lds_bytes"] == 16384 and shape["log2_buckets"] == 14
    else:
        assert shape["seeds_lds_bytes"] == 0 and shape["log2_buckets"] == 15
        h = isr.gram_hash_one(lsc.script(length)[w:w + N])
        assert int(isr.table_bucket([h], shape["log2_buckets"])[0]) == bucket
    _check_search(ix, c, want, ost, off, True)
    ix.close()


# ---- two workgroups of eight waves per CU, or one of sixteen -----------------------------------

def _device_bytes(ix, c, cap):
    """The device buffer of a search in each record form, as it lies there: the header's count
    and the records."""
    import torch
    out = []
    for packed, size in ((False, 32), (True, 16), (8, 8)):
        buf = torch.zeros(32 + cap * size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nw, _ = ix.search_end(ix.search_begin(c, buf.data_ptr(), cap, packed=packed, header=True))
        host = buf.cpu().numpy()
        assert int(host[:8].view(np.uint64)[0]) == nw
        out.append(host[:32 + nw * size].tobytes())
    return out


@pytest.mark.parametrize("length", lsc.TWO_PER_CU)
def test_two_workgroups_per_cu(base, oracle, length):
    """With several lanes k_scan_rows runs two 8-wave workgroups per CU while filter, seeds and
    per-wave state fit the CU's 160 KB of LDS twice: 2 * (filter + seeds + 1024 + sizeof(CoopLds)
    + 8 * sizeof(FusedLds)) <= 160 KB, i.e. filter + seeds <= 48,880 bytes.  At 32,777 tokens (G =
    32,771: 32 KB + 8 KB) it does; at 32,778 (G = 32,772: 32 KB + 16 KB) it misses by 272 bytes and
    runs one 16-wave workgroup per CU.  Both numbers follow from sizeof(FusedLds) = 3456,
    sizeof(CoopLds) = 4368 and the 160 KB limit: a change to the LDS layout moves them, and
    moves them here, knowingly.  The device buffer, with its header count, equals that of the
    same search with FS_ROWS_COOP=0 in every record form."""
    import torch
    tok, off = lsc.corpus(length)
    want, ost = oracle.rows(length, "plain", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, length)
    ix = _index(base, length, {"FS_LANES": "4"})
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d lanes 4" % length)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert shape["filter_log2_words"] == 13
    if length == lsc.TWO_PER_CU[0]:
        assert (shape["waves"], shape["blocks"], shape["seeds_lds_bytes"]) == (8, 2 * cus, 8192)
    else:
        assert (shape["waves"], shape["blocks"], shape["seeds_lds_bytes"]) == (16, cus, 16384)
    assert (shape["waves"], shape["blocks"] // cus) == isr.rows_waves(length, lsc.grams(length), N, 4)
    _check_search(ix, c, want, ost, off, True)
    dev = _device_bytes(ix, c, len(want) + 3)
    ix.close()
    plain = _index(base, length, {"FS_LANES": "4", "FS_ROWS_COOP": "0"})
    pc = plain.corpus(tok, off, base["chars"], base["off"])
    assert plain.scan_shape(pc)["waves"] == shape["waves"]
    assert dev == _device_bytes(plain, pc, len(want) + 3)
    assert dev[0][32:] == want.tobytes()
    plain.close()


# ---- a saturated filter: mostly false candidates -------------------------------------------------

@pytest.mark.parametrize("variant", ["one_lane", "lanes4"])
def test_saturated_filter(base, oracle, variant):
    """2^18 + 1 tokens and one long work drawn from the script's vocabulary: the 2^14-word
    filter has a bit density of about 0.4, so about 6 % of all windows are candidates that fail
    verification -- more than ten times the windows that match (test_index_shape_host.py counts
    both on the CPU; `matches` counts ten script windows for each of those).  The queue and
    the rounds of k_scan_rows work off mostly false candidates and the records are the
    oracle's."""
    L = lsc.EDGE + 1
    tok, off = lsc.saturated_batch(L)
    want, ost = oracle.rows(L, "saturated", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, L)
    passed = isr.sub_pass_count(tok, lsc.script(L), N)
    true = isr.matching_windows(tok, lsc.script(L), N)
    assert ost.matches == 10 * true and passed > 10 * true
    ix = _index(base, L, VARIANTS[variant])
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d %s, saturated" % (L, variant))
    assert shape["waves"] == 16 and shape["filter_log2_words"] == 14
    st = _check_search(ix, c, want, ost, off, False)
    print("candidates %d, filter passes restated %d, matching windows %d, matches %d"
          % (st.candidates, passed, true, st.matches))
    assert st.candidates == passed
    assert st.candidates > 10 * (st.matches // 10)
    ix.close()


# ---- the LSH pipeline with window numbers >= 2^18 -----------------------------------------------

def test_lsh_pipeline_past_2_18_windows(base, oracle):
    """2^18 + 40 tokens with mode = FS_MODE_GENERAL: window numbers >= 2^18 pass through the CSR
    buckets, the wildcard filter and the {key, window + 1} maps.  The records are the oracle's
    and, byte for byte, the exact pipeline's."""
    L = lsc.LSH_LENGTH
    tok, off = lsc.corpus(L)
    want, ost = oracle.rows(L, "plain", tok, off, base["chars"], base["off"])
    lsc.check_oracle_rows(want, L)
    assert int((want["orig_ix"] >= lsc.EDGE).sum()) >= 40
    ix = _index(base, L, {}, mode=abi.FS_MODE_GENERAL)
    assert ix.info["path"] == abi.FS_MODE_GENERAL
    c = ix.corpus(tok, off, base["chars"], base["off"])
    shape = _shape(ix, c, "%d general" % L)
    assert shape["waves"] == 0 and shape["host_wire8"] == 0
    got, st = ix.search(c)
    assert st.path == abi.FS_MODE_GENERAL
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
    ix.close()
    ex = _index(base, L, {})
    exact, est = ex.search(ex.corpus(tok, off, base["chars"], base["off"]))
    assert est.path == abi.FS_MODE_EXACT
    assert exact.tobytes() == got.tobytes()
    ex.close()
