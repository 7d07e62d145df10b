"""`pairs` on the GPU: fs_pairs / fs_pairs_rows against the restated contract
(tests/pairs_restated.py), every field of every work and pair compared for equality; numbers of
works, of column tiles and of script words around every size the kernels treat differently; the
planted copies of a synthetic corpus after a real search; `ao3.py pairs` byte for byte against
the oracle's two files."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, pairs, synth
from fandom_search_amd.cli import main
from tests import pairs_restated as pp
from tests.golden import make_pairs_golden as mpg
from tests.test_gpu_passages import expected_spans, repeated_ngrams

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fs_pairs.hip: works with a passage per tile of the coverage matrix (a workgroup takes a tile
# of rows against column tiles), column tiles per workgroup, 64-bit words per K-slice in LDS
TILE = 64
CHUNK = 8
K_SLICE = 32


def oracle(cols, n_works, n_script, m, g, s):
    recs = list(zip(*(c.tolist() for c in cols)))
    works, found = pp.pairs(recs, n_works, n_script, m, g, s)
    w = np.zeros(n_works, dtype=abi.PAIR_WORK_DTYPE)
    for name in pp.WORK_KEYS:
        w[name] = [d[name] for d in works]
    p = np.zeros(len(found), dtype=abi.PAIR_DTYPE)
    for name in pp.PAIR_KEYS:
        p[name] = [d[name] for d in found]
    return w, p


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.PAIR_WORK_DTYPE, abi.PAIR_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def records(sizes, n_script, seed, cont=0.93):
    """Records sorted by (work, fan_ix), sizes[w] of them in work w: diagonal steps most of the
    time (passages exist), repeats, jumps, script indices below n_script."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    work = np.repeat(np.arange(len(sizes)), sizes)
    fstep = rng.choice([0, 1, 2, 3], size=n, p=[0.05, 0.8, 0.1, 0.05])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < cont, fstep, rng.integers(-50, 50, size=n))
    orig = (np.cumsum(ostep) + int(rng.integers(0, 1 << 20))) % n_script
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32)


def from_spans(spans_of):
    """Records of works given as lists of (first script word, words): a diagonal run per span,
    the fan index jumping between them; an empty list is a work without records."""
    work, fan, orig = [], [], []
    for w, spans in enumerate(spans_of):
        f = 0
        for o0, k in spans:
            work += [w] * k
            fan += range(f, f + k)
            orig += range(o0, o0 + k)
            f += k + 10
    return tuple(np.array(c, dtype=np.uint32) for c in (work, fan, orig))


def check(cols, n_works, n_script, m=6, g=0, s=6):
    got = pairs.find_pairs(*cols, n_works, n_script, m, g, s)
    assert_equal(got, oracle(cols, n_works, n_script, m, g, s))
    return got


def test_no_records_and_one_record():
    empty = (np.zeros(0, np.uint32),) * 3
    works, found = check(empty, 3, 10)
    assert works.tolist() == [(0, 0, abi.FS_NONE, 0)] * 3 and len(found) == 0
    works, found = check(empty, 0, 0)
    assert len(works) == 0 and len(found) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32))
    works, found = check(one, 3, 10, m=1, s=1)
    assert works.tolist() == [(0, 0, abi.FS_NONE, 0), (1, 0, abi.FS_NONE, 0),
                              (0, 0, abi.FS_NONE, 0)] and len(found) == 0
    works, found = check(one, 3, 10, m=2, s=1)
    assert not works["covered"].any()


def interleaved(n_active, spans_of_active, seed):
    """Works without a passage (no records, or a run one short of three words) between the
    active ones, so that the active numbering differs from the work numbering."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_active):
        for _ in range(int(rng.integers(0, 3))):
            out.append([(int(rng.integers(0, 200)), 2)] if rng.random() < 0.5 else [])
        out.append(spans_of_active(k, rng))
    out.append([])
    return out


@pytest.mark.parametrize("n_active", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_active_works_around_the_tile(n_active):
    n_script = 300
    spans_of = interleaved(n_active, lambda k, rng: [
        (int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))
        for _ in range(int(rng.integers(1, 4)))], seed=n_active)
    cols = from_spans(spans_of)
    assert len(spans_of) > n_active + 1
    works, found = check(cols, len(spans_of), n_script, m=3, s=1)
    assert (works["covered"] > 0).sum() == n_active
    check(cols, len(spans_of), n_script, m=3, s=4)
    # every work covers the same ten words: every pair is kept, the diagonal tiles keep a < b
    # only and nothing twice
    spans_of = interleaved(n_active, lambda k, rng: [(120, 10)], seed=n_active + 1000)
    works, found = check(from_spans(spans_of), len(spans_of), n_script, m=3, s=10)
    assert len(found) == n_active * (n_active - 1) // 2
    assert (found["a"] < found["b"]).all()
    assert len(set(zip(found["a"].tolist(), found["b"].tolist()))) == len(found)
    active = works["covered"] > 0
    assert (works["partners"][active] == n_active - 1).all() and not works["partners"][~active].any()


@pytest.mark.parametrize("tiles", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_column_tiles_around_a_chunk(tiles):
    n_active = (tiles - 1) * TILE + 5
    rng = np.random.default_rng(tiles)
    spans_of = [[(int(rng.integers(0, 59)), int(rng.integers(1, 3)))] for _ in range(n_active)]
    cols = from_spans(spans_of)
    works, found = check(cols, n_active, 60, m=1, s=1)
    assert len(found) > 1000 and found["b"].max() == n_active - 1
    check(cols, n_active, 60, m=1, s=2)


@pytest.mark.parametrize("n_script", [1, 63, 64, 65, 64 * K_SLICE - 1, 64 * K_SLICE,
                                      64 * K_SLICE + 1, 128 * K_SLICE - 1, 128 * K_SLICE,
                                      128 * K_SLICE + 1])
def test_script_sizes_around_a_word_and_a_slice(n_script):
    sizes = np.random.default_rng(n_script).integers(0, 60, size=70)
    sizes[[3, 66]] = 5
    cols = records(sizes, n_script, seed=n_script)
    # the last script word, the last bit of the last 64-bit word, covered by two works
    for w in (3, 66):
        at = int(np.nonzero(cols[0] == w)[0][0])
        cols[2][at] = n_script - 1
    works, found = check(cols, 70, n_script, m=1, s=1)
    last = [p for p in found if (p["a"], p["b"]) == (3, 66)]
    assert len(last) == 1 and last[0]["last"] == n_script - 1
    if n_script > 1:
        check(cols, 70, n_script, m=3, g=1, s=2)


def test_a_shared_run_across_a_word_boundary():
    n_script = 200
    spans_of = [[(60, 11)],                      # 60..70, across the bit 63 | 64
                [(50, 30)],
                [(192, 8)],                      # up to the last script word
                [(120, 80)],
                [(10, 5), (30, 5), (127, 2)],    # two runs of equal length: the first one
                [(0, 200)]]
    works, found = check(from_spans(spans_of), 6, n_script, m=2, s=1)
    by = {(int(p["a"]), int(p["b"])): p for p in found}
    assert (by[0, 1]["run_first"], by[0, 1]["run_words"]) == (60, 11)
    assert (by[2, 3]["run_first"], by[2, 3]["run_words"], by[2, 3]["last"]) == (192, 8, 199)
    assert (by[4, 5]["run_first"], by[4, 5]["run_words"], by[4, 5]["shared"]) == (10, 5, 12)
    assert (by[3, 4]["run_first"], by[3, 4]["run_words"]) == (127, 2)
    assert (by[3, 5]["run_first"], by[3, 5]["run_words"]) == (120, 80)   # over two boundaries


def test_min_shared_sweep_over_one_input():
    sizes = np.random.default_rng(12).integers(0, 80, size=150)
    cols = records(sizes, 400, seed=12)
    works, found = check(cols, 150, 400, m=3, s=1)
    top = int(found["shared"].max())
    assert top > 6 and len(found) > 100
    works6, found6 = check(cols, 150, 400, m=3, s=6)
    assert 0 < len(found6) < len(found)
    assert (works6["partners"] <= works["partners"]).all()
    assert works6["partners"].sum() == 2 * len(found6)
    none = works6["partners"] == 0
    assert none.any() and (works6["best"][none] == abi.FS_NONE).all()
    worksx, foundx = check(cols, 150, 400, m=3, s=top + 1)
    assert len(foundx) == 0 and not worksx["partners"].any()
    assert (worksx["best"] == abi.FS_NONE).all() and (worksx["covered"] == works["covered"]).all()


def _call(L, cols, n_works, n_script, m, s, works, found, cap, n, n_rows=None):
    return L.fs_pairs(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                      abi.ptr(cols[2], C.c_uint32), len(cols[0]) if n_rows is None else n_rows,
                      n_works, n_script, m, 0, s, works.ctypes.data_as(C.c_void_p),
                      found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


def test_capacity_too_small_by_one_exact_and_zero():
    sizes = np.random.default_rng(8).integers(0, 80, size=100)
    cols = [np.ascontiguousarray(c) for c in records(sizes, 300, seed=8)]
    want = oracle(cols, 100, 300, 3, 0, 2)
    k = len(want[1])
    assert k > 10
    L = _lib.load()
    works = np.zeros(100, dtype=abi.PAIR_WORK_DTYPE)
    found = np.zeros(k, dtype=abi.PAIR_DTYPE)
    n = C.c_uint64(0)
    for cap in (k - 1, 0):
        works[:] = 0
        assert _call(L, cols, 100, 300, 3, 2, works, found, cap, n) == abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((works, want[1]), want)               # the works are complete
        assert not found["b"].any()                        # the pairs untouched
    assert _call(L, cols, 100, 300, 3, 2, works, found, k, n) == abi.FS_OK and n.value == k
    assert_equal((works, found), want)


def test_refusals():
    """include/fandom_search.h.  The accepted side of FS_PAIRS_MAX_BYTES, a coverage matrix of
    1 GiB, is not tested: only that one 64-bit word more is refused."""
    cols = records([300, 500, 200], 1000, seed=9)

    def refused(c, n_works=3, n_script=1000, m=6, s=6, code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            pairs.find_pairs(*c, n_works, n_script, m, 0, s)
        assert e.value.code == code
    refused(cols, m=0)
    refused(cols, s=0)
    refused(cols, n_works=2)                               # a work >= n_works
    refused(cols, n_script=int(cols[2].max()))             # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))
    far = cols[2].copy()                                   # ... on a stray record
    far[:] = np.arange(1000) % 900
    far[20] = 1000
    refused((cols[0], np.arange(1000, dtype=np.uint32) * 3, far))
    refused(cols, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED)
    L = _lib.load()
    n = C.c_uint64(0)
    works = np.zeros(3, dtype=abi.PAIR_WORK_DTYPE)
    rc = _call(L, cols, 3, 1000, 6, 6, works, works, 0, n, n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(cols, 3, 1000)                                   # and the same columns are accepted
    # 16 385 works of one record each, a passage at --min-words 1, over 2^19 script words:
    # 16 385 rows of 8 192 words of 8 bytes, one row above FS_PAIRS_MAX_BYTES
    many = abi.FS_PAIRS_MAX_BYTES // ((1 << 19) // 8) + 1
    assert many == 16385
    one = (np.arange(many, dtype=np.uint32), np.zeros(many, np.uint32),
           np.arange(many, dtype=np.uint32) % 5000)
    refused(one, n_works=many, n_script=1 << 19, m=1, s=1, code=abi.FS_E_UNSUPPORTED)
    works, found = pairs.find_pairs(*one, many, 5000, 1, 0, 1)   # the same columns, accepted
    # 1 385 script words are held by four works each, 3 615 by three
    assert (works["covered"] == 1).all() and len(found) == 1385 * 6 + 3615 * 3


# ---- after a real search ---------------------------------------------------------------

def test_device_rows_after_a_search(synth_base):
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    vocab, emb = synth_base["words"], synth_base["emb"]
    n_works, per, n = 300, 2000, 6
    script = synth.script_tokens(5000)
    tok, off = synth.corpus_tokens(n_works, per, script)
    ix = ScriptIndex(script, [vocab[int(t)] for t in script], emb, synth.lsh_normals(n))
    corpus = ix.corpus(tok, off, synth_base["chars"], synth_base["off"])
    cap = len(tok) // 4
    buf = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    n_rows, _ = ix.search_device(corpus, buf.data_ptr(), cap)
    rows = buf[:n_rows * 32].cpu().numpy().view(abi.ROW_DTYPE)
    cols = tuple(np.ascontiguousarray(rows[c]) for c in ("work", "fan_ix", "orig_ix"))
    for g, s in ((0, 6), (1, 1)):
        dev = ix.pairs_device(buf.data_ptr(), n_rows, n_works, n, g, s)
        host = pairs.find_pairs(*cols, n_works, len(script), n, g, s)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, len(script), n, g, s))
        if (g, s) == (0, 6):
            first = dev
    # the caller's own device buffers, the pairs' too small by one first
    works, found = first
    k = len(found)
    assert k > 10
    d_works = torch.zeros(n_works * 16, dtype=torch.uint8, device="cuda")
    d_pairs = torch.zeros(k * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_works.data_ptr(), d_pairs.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        ix.pairs_device(buf.data_ptr(), n_rows, n_works, n, 0, 6, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_works.cpu().numpy().view(abi.PAIR_WORK_DTYPE) == works).all()
    assert not d_pairs.cpu().numpy().any()
    assert ix.pairs_device(buf.data_ptr(), n_rows, n_works, n, 0, 6, out_ptrs=ptrs, cap=k) == k
    assert (d_pairs.cpu().numpy().view(abi.PAIR_DTYPE) == found).all()
    # no records: works without coverage on the device
    assert ix.pairs_device(buf.data_ptr(), 0, n_works, n, 0, 6, out_ptrs=ptrs, cap=k) == 0
    none = d_works.cpu().numpy().view(abi.PAIR_WORK_DTYPE)
    assert (none["best"] == abi.FS_NONE).all() and not none["covered"].any()
    # two works planted with the same verbatim span of the script form a kept pair whose
    # shared words contain the overlap; where the longest run is elsewhere it is no shorter
    repeated = repeated_ngrams(script, n)
    planted = []
    for w in range(n_works):
        planted += [(src, src + length, w) for _, length, src in
                    expected_spans(w, per, script, n, repeated)[0] if length >= n]
    by = {(int(p["a"]), int(p["b"])): p for p in found}
    checked = 0
    for i, (s0, e0, w0) in enumerate(planted):
        for s1, e1, w1 in planted[i + 1:]:
            lo, hi = max(s0, s1), min(e0, e1)
            if w0 == w1 or hi - lo < n:
                continue
            p = by[min(w0, w1), max(w0, w1)]
            assert p["first"] <= lo and p["last"] >= hi - 1 and p["run_words"] >= hi - lo
            if s0 == s1 and e0 == e1:
                assert p["shared"] >= e0 - s0
                if p["run_words"] == e0 - s0:
                    assert p["run_first"] <= s0             # (the first among equals)
            checked += 1
    assert checked > 20
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

def _run_command(tmp_path, src_path, m, g, s, reader):
    prefix = str(tmp_path / "p")
    assert main(["pairs", src_path, "-o", prefix, "--min-words", str(m), "--max-gap", str(g),
                 "--min-shared", str(s), "--reader", reader]) == 0
    return tuple(open(p, "rb").read() for p in pairs.output_names(src_path, prefix))


@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,src,m,g,s", mpg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g, s, reader):
    got = _run_command(tmp_path, os.path.join(GOLDEN, src), m, g, s, reader)
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        want = pp.pairs_csv(fh.read(), m, g, s)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mpg.golden_names(case, m, g, s), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_search_then_pairs(tmp_path, monkeypatch, synth_base):
    from fandom_search_amd import search
    vocab = synth_base["words"]
    n_works, per = 40, 1500
    script = synth.script_tokens(3000)
    fandir = tmp_path / "fanworks"
    synth.write_corpus(str(fandir), n_works, per, script, vocab)
    (tmp_path / "script.txt").write_text(synth.script_markup(script, vocab))
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    monkeypatch.delenv("FANDOM_SEARCH_VECTORS", raising=False)
    assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--synthetic-vocab"]) == 0
    dated = "match-6gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    assert main(["pairs", dated, "--min-shared", "1"]) == 0   # default prefix: beside the input
    with open(dated, newline="", encoding="utf-8") as fh:
        want = pp.pairs_csv(fh.read(), min_shared=1)
    for path, text in zip(pairs.output_names(dated), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[1].count("\r\n") > 10
