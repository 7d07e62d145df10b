"""`quotes` on the GPU: fs_quotes / fs_quotes_rows against the restated contract
(tests/quotes_restated.py), every field of every word and region compared for equality; works
of every size the kernels treat differently; the planted copies of a synthetic corpus after a
real search; `ao3.py quotes` byte for byte against the oracle's two files."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, quotes, synth
from fandom_search_amd.cli import main
from tests import quotes_restated as qr
from tests.golden import make_quotes_golden as mqg
from tests.test_gpu_passages import expected_spans, repeated_ngrams

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# records of a work one wave reduces; longer works are cut into slices.  Doubled until it is at
# least 2.5 bits-words of the script, 2.5 * n_script / 32 (65536 at the limit below)
SLICE = 8192
WORKS_PER_WAVE = 8          # consecutive works a wave takes from MANY_WORKS works on, one below
MANY_WORKS = 1 << 18


def oracle(cols, n_works, n_script, m, g, k):
    work, fan, orig, comb = cols
    recs = list(zip(work.tolist(), fan.tolist(), orig.tolist(), [0.0] * len(work), comb.tolist()))
    words, regions = qr.quotes(recs, n_works, n_script, m, g, k)
    w = np.zeros(n_script, dtype=abi.QUOTE_WORD_DTYPE)
    for name in qr.WORD_KEYS:
        w[name] = [d[name] for d in words]
    r = np.zeros(len(regions), dtype=abi.QUOTE_REGION_DTYPE)
    for name in qr.REGION_KEYS:
        r[name] = [d[name] for d in regions]
    return w, r


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.QUOTE_WORD_DTYPE, abi.QUOTE_REGION_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def records(sizes, n_script, seed, cont=0.8, nan=0.02):
    """Records sorted by (work, fan_ix), sizes[w] of them in work w: diagonal steps most of the
    time, repeats, jumps, NaN, -0.0 and 0.0, script indices below n_script."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    work = np.repeat(np.arange(len(sizes)), sizes)
    fstep = rng.choice([0, 1, 2, 3], size=n, p=[0.05, 0.8, 0.1, 0.05])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < cont, fstep, rng.integers(-50, 50, size=n))
    orig = (np.cumsum(ostep) + int(rng.integers(0, 1 << 20))) % n_script
    comb = np.round(rng.random(n) * 0.6, 2) * rng.integers(0, 2, size=n)
    r = rng.random(n)
    comb[r < nan] = np.nan
    comb[(r >= nan) & (r < 2 * nan)] = -0.0
    comb[(r >= 2 * nan) & (r < 3 * nan)] = 0.05
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), comb


def check(cols, n_works, n_script, m=6, g=0, k=1):
    got = quotes.find_quotes(*cols, n_works, n_script, m, g, k)
    assert_equal(got, oracle(cols, n_works, n_script, m, g, k))
    return got


def test_no_records_and_one_record():
    empty = (np.zeros(0, np.uint32),) * 3 + (np.zeros(0),)
    words, regions = check(empty, 3, 10)
    assert len(words) == 10 and (words["region"] == abi.FS_NONE).all() and len(regions) == 0
    words, regions = check(empty, 0, 0)
    assert len(words) == 0 and len(regions) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32),
           np.array([-0.0]))
    words, regions = check(one, 3, 10, m=1)
    assert words[9].tolist() == (1, 1, 1, 1, 1, 0)
    assert regions.tolist() == [(9, 9, 1, 1, 1, 1, 1, 9, 9, 0)]
    words, regions = check(one, 3, 10, m=2)
    assert words[9].tolist() == (1, 1, 1, 0, 0, abi.FS_NONE) and len(regions) == 0


def test_random_records_over_the_parameters():
    rng = np.random.default_rng(2026)
    seen = set()
    for j in range(14):
        n_works = int(rng.integers(1, 400))
        sizes = rng.integers(0, 300, size=n_works) * (rng.random(n_works) < 0.8)
        n_script = int(rng.integers(1, 30_000)) if j % 3 else int(rng.integers(1, 600))
        cols = records(sizes, n_script, seed=j, cont=float(rng.random()) * 0.5 + 0.5,
                       nan=float(rng.random()) * 0.2)
        m, g = int(rng.integers(1, 13)), int(rng.integers(0, 4))
        for k in (1, int(rng.integers(2, 6))):
            _, regions = check(cols, n_works, n_script, m, g, k)
            seen.add((k > 1, len(regions) > 0))
    assert seen >= {(False, True), (True, True)}          # regions at one work and at several


def test_min_works_above_every_depth_gives_no_regions():
    cols = records([300, 200, 0, 500], 800, seed=4, cont=0.95)
    words, regions = check(cols, 4, 800, m=3, k=1)
    assert len(regions) > 0 and 1 <= words["n_passage_works"].max() <= 3
    words, regions = check(cols, 4, 800, m=3, k=int(words["n_passage_works"].max()) + 1)
    assert len(regions) == 0 and (words["region"] == abi.FS_NONE).all()


def test_a_hundred_thousand_small_works():
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 6, size=100_000)
    cols = records(sizes, 20_000, seed=5, cont=0.95)
    for k in (1, 3):
        words, regions = check(cols, len(sizes), 20_000, m=3, k=k)
        assert words["n_words"].sum() == sizes.sum() and len(regions) > (100 if k > 1 else 0)


def test_one_work_of_three_million_records():
    n = 3_000_000
    cols = records([0, n, 0], 20_000, seed=3, cont=0.97)
    words, regions = check(cols, 3, 20_000)
    assert words["n_words"].sum() == n and (words["n_works"] == 1).all()
    assert words["n_passage_works"].max() == 1 and regions["n_works"].tolist() == [1] * len(regions)
    assert regions["n_passages"].sum() > 10_000


@pytest.mark.parametrize("size", [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE,
                                  2 * SLICE + 1, 5 * SLICE + 3])
def test_works_that_end_around_a_slice(size):
    # the work alone; between small works, so that it starts anywhere in a slice; and twice in
    # a row, so that one slice holds the end of one large work and the start of the next
    for sizes in ([size], [3, 0, size, 5], [SLICE // 2 + 1, size, size, 2, SLICE + 1, 7]):
        cols = records(sizes, 5000, seed=size, cont=0.9)
        check(cols, len(sizes), 5000, k=1)
        check(cols, len(sizes), 5000, m=4, g=1, k=2)


@pytest.mark.parametrize("n_works", [1, WORKS_PER_WAVE + 1, 65, 4097, MANY_WORKS - 1,
                                     MANY_WORKS + WORKS_PER_WAVE + 1])
def test_numbers_of_works_around_a_wave_share(n_works):
    rng = np.random.default_rng(n_works)
    sizes = rng.integers(0, 40 if n_works < 10_000 else 4, size=n_works)
    cols = records(sizes, 3000, seed=n_works, cont=0.95)
    check(cols, n_works, 3000, m=2, g=1, k=1)
    check(cols, n_works, 3000, m=2, g=1, k=3)


@pytest.mark.parametrize("n_script", [1, (1 << 19) - 1, 1 << 19])
def test_script_sizes_up_to_the_limit(n_script):
    # (at the limit a slice is 65536 records: works on both sides of it)
    cols = records([40, 20_000, 0, 3, 65_536, 65_537, 140_000], n_script, seed=n_script, cont=0.9)
    check(cols, 7, n_script, k=1)
    if n_script > 1:                                    # the last script word, too
        cols[2][-1] = n_script - 1
        cols[2][5] = n_script - 1
        words, _ = check(cols, 7, n_script, m=1, k=2)
        assert words["n_words"][n_script - 1] >= 2


def test_past_the_limit_is_refused():
    """include/fandom_search.h: n_script > FS_WORKS_MAX_SCRIPT is FS_E_UNSUPPORTED (no slower
    form)."""
    cols = records([100], 1000, seed=1)
    with pytest.raises(_lib.FsError) as e:
        quotes.find_quotes(*cols, 1, (1 << 19) + 1)
    assert e.value.code == abi.FS_E_UNSUPPORTED
    L = _lib.load()
    n = C.c_uint64(0)
    words = np.zeros(1000, dtype=abi.QUOTE_WORD_DTYPE)
    rc = L.fs_quotes(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                     abi.ptr(cols[2], C.c_uint32), abi.ptr(cols[3], C.c_double), 1 << 32, 1, 1000,
                     6, 0, 1, words.ctypes.data_as(C.c_void_p), None, 0, C.byref(n))
    assert rc == abi.FS_E_UNSUPPORTED                    # (refused before a record is read)


def test_refusals():
    cols = records([3000, 5000, 2000], 1000, seed=9)

    def refused(c, n_works=3, n_script=1000, m=6, k=1):
        with pytest.raises(_lib.FsError) as e:
            quotes.find_quotes(*c, n_works, n_script, m, 0, k)
        assert e.value.code == abi.FS_E_INVALID
    refused(cols, m=0)
    refused(cols, k=0)
    refused(cols, n_works=2)                               # a work >= n_works
    refused(cols, n_works=0)
    refused(cols, n_script=int(cols[2].max()))             # an orig_ix >= n_script
    refused(cols, n_script=0)
    fan = cols[1].copy()
    fan[7000], fan[7001] = fan[7001] + 1, fan[7000]
    refused((cols[0], fan, cols[2], cols[3]))
    work = cols[0].copy()
    work[9000] = 0
    refused((work, np.arange(10_000, dtype=np.uint32), cols[2], cols[3]))
    # an orig_ix outside the script at the end of a passage, and on a stray record
    far = cols[2].copy()
    far[:] = np.arange(10_000) % 900
    far[20] = 1000
    refused((cols[0], np.arange(10_000, dtype=np.uint32), far, cols[3]))
    check(cols, 3, 1000)                                   # and the same columns are accepted


def test_capacity_too_small_by_one_exact_and_zero():
    cols = [np.ascontiguousarray(c) for c in records([300, 0, 4000, 20_000], 3000, seed=8,
                                                     cont=0.9)]
    want = oracle(cols, 4, 3000, 6, 0, 1)
    k = len(want[1])
    assert k > 10
    L = _lib.load()
    words = np.zeros(3000, dtype=abi.QUOTE_WORD_DTYPE)
    regions = np.zeros(k, dtype=abi.QUOTE_REGION_DTYPE)
    n = C.c_uint64(0)

    def call(cap):
        return L.fs_quotes(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                           abi.ptr(cols[2], C.c_uint32), abi.ptr(cols[3], C.c_double),
                           len(cols[0]), 4, 3000, 6, 0, 1, words.ctypes.data_as(C.c_void_p),
                           regions.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))
    for cap in (k - 1, 0):
        words[:] = 0
        assert call(cap) == abi.FS_E_CAPACITY and n.value == k
        assert_equal((words, want[1]), want)               # the words are complete
        assert not regions["last"].any()
    assert call(k) == abi.FS_OK and n.value == k
    assert_equal((words, regions), want)


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
    cols = tuple(np.ascontiguousarray(rows[c]) for c in ("work", "fan_ix", "orig_ix", "comb"))
    for g, k in ((0, 1), (1, 1), (0, 2), (1, 4)):
        dev = ix.quotes_device(buf.data_ptr(), n_rows, n_works, n, g, k)
        host = quotes.find_quotes(*cols, n_works, len(script), n, g, k)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, len(script), n, g, k))
        if (g, k) == (0, 1):
            first = dev
    # the caller's own device buffers, the regions' too small first
    words, regions = first
    k = len(regions)
    d_words = torch.zeros(len(script) * 24, dtype=torch.uint8, device="cuda")
    d_regions = torch.zeros(k * 40, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_words.data_ptr(), d_regions.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        ix.quotes_device(buf.data_ptr(), n_rows, n_works, n, 0, 1, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_words.cpu().numpy().view(abi.QUOTE_WORD_DTYPE) == words).all()
    assert ix.quotes_device(buf.data_ptr(), n_rows, n_works, n, 0, 1, out_ptrs=ptrs, cap=k) == k
    assert (d_regions.cpu().numpy().view(abi.QUOTE_REGION_DTYPE) == regions).all()
    # no records: zeroed words on the device
    assert ix.quotes_device(buf.data_ptr(), 0, n_works, n, 0, 1, out_ptrs=ptrs, cap=k) == 0
    none = d_words.cpu().numpy().view(abi.QUOTE_WORD_DTYPE)
    assert (none["region"] == abi.FS_NONE).all() and not none["n_words"].any()
    # every planted verbatim span of at least n words lies inside one region
    checked = 0
    repeated = repeated_ngrams(script, n)
    for w in range(n_works):
        for dst, length, src in expected_spans(w, per, script, n, repeated)[0]:
            inside = words["region"][src:src + length]
            assert length >= n and inside[0] != abi.FS_NONE and (inside == inside[0]).all(), (w, dst)
            assert (words["n_passage_works"][src:src + length] >= 1).all()
            checked += 1
    assert checked > 200
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

def _run_command(tmp_path, src_path, m, g, k):
    prefix = str(tmp_path / "q")
    assert main(["quotes", src_path, "-o", prefix, "--min-words", str(m), "--max-gap", str(g),
                 "--min-works", str(k)]) == 0
    return tuple(open(p, "rb").read() for p in quotes.output_names(src_path, prefix))


@pytest.mark.parametrize("case,src,m,g,k", mqg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g, k):
    got = _run_command(tmp_path, os.path.join(GOLDEN, src), m, g, k)
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        want = qr.quotes_csv(fh.read(), m, g, k)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mqg.golden_names(case, m, g, k), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_search_then_quotes(tmp_path, monkeypatch, synth_base):
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
    assert main(["quotes", dated]) == 0                    # default prefix: beside the input
    with open(dated, newline="", encoding="utf-8") as fh:
        want = qr.quotes_csv(fh.read())
    for path, text in zip(quotes.output_names(dated), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[0].count("\r\n") > 10 and want[1].count("\r\n") > 100
