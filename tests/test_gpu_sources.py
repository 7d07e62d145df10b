"""`sources` on the GPU: fs_sources against the restated contract (tests/sources_restated.py),
every field of every passage, (work, script) row, script and pair compared for equality, every
case down each forced path in turn (FS_SOURCES_UNION, FS_SOURCES_PACK, FS_SOURCES_DENSE); the
number of files around every packing edge, the passages of one (work, script) around the lane,
wave and workgroup edges; `ao3.py sources` byte for byte against the committed files, and behind
a several-script `ao3.py search`.

A file is a list of passages (work, first fan word, words[, exact words]) in (work, fan) order;
the script words of two passages never follow one another, so no two of them join."""

import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, passages, search, sources, synth
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests import sources_restated as sr
from tests.golden import make_sources_golden as msg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
TOP = 0xFFFFFFFF
DTYPES = (abi.SOURCE_PASSAGE_DTYPE, abi.SOURCE_WORK_DTYPE, abi.SOURCE_SCRIPT_DTYPE,
          abi.SOURCE_PAIR_DTYPE)
# (FS_SOURCES_UNION, FS_SOURCES_PACK, FS_SOURCES_DENSE)
PATHS = {"default": (None, None, None), "union": ("1", None, None), "wave": (None, "0", None),
         "global": (None, None, "0"), "all": ("1", "0", "0")}


@pytest.fixture(params=list(PATHS), ids=list(PATHS))
def path(request, monkeypatch):
    for name, value in zip(("FS_SOURCES_UNION", "FS_SOURCES_PACK", "FS_SOURCES_DENSE"),
                           PATHS[request.param]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


def columns(spans):
    """(work, fan_ix, orig_ix, comb) of one file's passages."""
    cols, orig = [[], [], [], []], 0
    for item in spans:
        work, fan, words = item[:3]
        exact = item[3] if len(item) > 3 else words
        cols[0] += [work] * words
        cols[1] += range(fan, fan + words)
        cols[2] += range(orig, orig + words)
        cols[3] += [0.0 if k < exact else 0.25 for k in range(words)]
        orig += words + 5
    return (np.asarray(cols[0], dtype=np.uint32), np.asarray(cols[1], dtype=np.uint32),
            np.asarray(cols[2], dtype=np.uint32), np.asarray(cols[3], dtype=np.float64))


def oracle(files, min_words=6, max_gap=0):
    recs = [list(zip(w.tolist(), f.tolist(), o.tolist(), c.tolist(), c.tolist()))
            for w, f, o, c in files]
    tabs = sr.as_tuples(sr.sources(recs, min_words, max_gap))
    return tuple(np.array(t, dtype=dt) for t, dt in zip(tabs, DTYPES))


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert a.dtype == dt and len(a) == len(b), (dt.names[:2], len(a), len(b))
        for name in dt.names:
            bad = np.flatnonzero(a[name] != b[name])
            assert not len(bad), (name, bad[:5], a[name][bad[:5]], b[name][bad[:5]])
    ps, ws, ss, qs = got
    assert (ss["alone"] + ss["won"] + ss["lost"] == ss["passages"]).all()
    assert (ws["alone"] + ws["won"] + ws["lost"] == ws["passages"]).all()
    assert (qs["a_wins"] + qs["b_wins"] == qs["contests"]).all()
    assert (ps["contested_words"] + ps["sole_words"]
            == ps["fan_last"].astype(np.int64) - ps["fan_first"] + 1).all()
    assert ss["passages"].sum() == len(ps) and ss["works"].sum() == len(ws)
    assert ps["rivals"].sum() == 2 * qs["contests"].sum()
    assert ws["primary"].sum() == len(np.unique(ws["work"]))
    key = (ps["work"].astype(np.int64) << 32) | ps["fan_first"]
    assert (np.diff(key) >= 0).all()
    for w in np.unique(ps["work"][ps["rivals"] > 0]):         # a work with a contest has a winner
        assert (ps["outcome"][ps["work"] == w] == abi.FS_SOURCE_WON).any()


def check(spans_of, n_works, min_words=6, max_gap=0, want=None):
    files = [columns(s) for s in spans_of]
    if want is None:
        want = oracle(files, min_words, max_gap)
    got = sources.find_sources(files, n_works, min_words, max_gap)
    assert_equal(got, want)
    return got


# ---- the number of files: the packing edges ---------------------------------------------

def planted(K, n_works, seed, anchors=4, fill=0.6):
    """K files over n_works works: per work `anchors` places 40 fan words apart, where a script
    has, with probability `fill`, a passage of 6..14 words starting up to 9 words in."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(K):
        spans = []
        for w in range(n_works):
            for a in range(anchors):
                if rng.random() < fill:
                    words = int(rng.integers(6, 15))
                    spans.append((w, 40 * a + int(rng.integers(0, 10)), words,
                                  words - int(rng.integers(0, 3))))
        out.append(spans)
    return out


@functools.lru_cache(maxsize=None)
def k_case(K):
    spans = planted(K, 5, seed=K, anchors=3, fill=0.9 if K < 8 else 0.25)
    return spans, oracle([columns(s) for s in spans])


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64])
def test_files_around_every_packing_edge(path, K):
    spans, want = k_case(K)
    ps, ws, ss, qs = check(spans, 5, want=want)
    assert len(ss) == K and len(qs) == K * (K - 1) // 2 and len(ps) > 0
    if K == 1:
        assert (ps["outcome"] == abi.FS_SOURCE_ALONE).all() and (ps["best_rival"] == NONE).all()
        w, f, o, c = columns(spans[0])
        alone = passages.find_passages(w, f, o, c, c)
        for name in ("first", "n_words", "n_exact"):
            assert (ps[name] == alone[name]).all()
    else:
        assert qs["contests"].sum() > 0 and ps["rival_scripts"].max() <= K - 1
    if K >= 3:
        assert (ps["rival_scripts"] >= 2).any()               # the union pass has work


# ---- the passages of one (work, script) ------------------------------------------------

@functools.lru_cache(maxsize=None)
def list_case(m, rivals):
    """Script 0: m passages of 6 words every 10 fan words in work 1.  Script 1: one passage over
    the last two of them, or 300 of 2 words every 9; script 2: a passage every 70 words; works
    0 and 2 hold a passage of each script at work 1's first fan words: rivals of one another,
    not of work 1's."""
    edge = [(0, 0, 6), (2, 0, 6)]
    a = edge[:1] + [(1, 10 * i, 6) for i in range(m)] + edge[1:]
    if rivals == 1:
        b = edge[:1] + [(1, max(0, 10 * (m - 2)) + 3, 12)] + edge[1:]
    else:
        b = edge[:1] + [(1, 9 * j + 1, 2) for j in range(300)] + edge[1:]
    c = edge[:1] + [(1, 70 * j + 4, 3, 2) for j in range(m // 7 + 1)] + edge[1:]
    spans = (a, b, c)
    return spans, oracle([columns(s) for s in spans], min_words=2)


@pytest.mark.parametrize("rivals", [1, 300])
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257])
def test_m_passages_of_one_work_and_script(path, m, rivals):
    spans, want = list_case(m, rivals)
    ps, ws, ss, qs = check(spans, 3, min_words=2, want=want)
    assert ss["passages"][0] == m + 2 and ss["passages"][1] == rivals + 2
    row = ws[(ws["work"] == 1) & (ws["script"] == 0)][0]
    assert row["passages"] == m and row["covered_words"] == 6 * m
    assert qs["works_both"].tolist() == [3, 3, 3]


# ---- span geometry ------------------------------------------------------------------------

def test_identical_nested_touching_and_adjacent_spans(path):
    a = [(0, 10, 8), (1, 10, 12), (2, 10, 6), (3, 10, 6), (4, 10, 6), (5, 10, 6, 5)]
    b = [(0, 10, 8), (1, 12, 6), (2, 15, 6), (3, 16, 6), (5, 10, 6)]
    ps, ws, ss, qs = check([a, b], 6)
    got = {(int(p["work"]), int(p["script"])): p for p in ps}
    assert [int(got[(0, s)]["outcome"]) for s in (0, 1)] == [abi.FS_SOURCE_WON, abi.FS_SOURCE_LOST]
    assert (got[(0, 0)]["contested_words"], got[(0, 0)]["sole_words"]) == (8, 0)      # identical
    assert (got[(1, 0)]["contested_words"], got[(1, 0)]["sole_words"]) == (6, 6)      # nested
    assert (got[(1, 1)]["contested_words"], got[(1, 1)]["sole_words"]) == (6, 0)
    assert (got[(2, 0)]["contested_words"], got[(2, 1)]["contested_words"]) == (1, 1)  # touching
    assert (got[(3, 0)]["rivals"], got[(3, 1)]["rivals"]) == (0, 0)                   # adjacent
    assert int(got[(4, 0)]["outcome"]) == abi.FS_SOURCE_ALONE                         # one file only
    assert int(got[(5, 1)]["outcome"]) == abi.FS_SOURCE_WON                           # exact words
    assert qs[0].tolist() == (0, 1, 5, 0, 4, 21, 3, 1)


def test_one_rival_over_three_and_three_rivals_over_one(path):
    # work 0: script 1 covers three passages of script 0; work 1: three scripts (and script 1
    # twice) on one passage of script 0; work 2: the fan words of work 1 again, script 0 alone
    a = [(0, 0, 6), (0, 10, 6), (0, 20, 6), (1, 0, 30), (2, 0, 30)]
    b = [(0, 3, 20), (1, 2, 6), (1, 20, 8)]
    c = [(1, 5, 10), (3, 0, 6)]
    d = [(1, 12, 10, 9), (3, 0, 6)]
    ps, ws, ss, qs = check([a, b, c, d], 4)
    one = ps[(ps["work"] == 1) & (ps["script"] == 0)][0]
    assert (one["rivals"], one["rival_scripts"], one["outcome"]) == (4, 3, abi.FS_SOURCE_WON)
    assert (one["contested_words"], one["sole_words"]) == (26, 4)     # words 2 .. 27
    assert (one["best_rival"], one["best_rival_words"], one["best_rival_fan_first"]) == (2, 10, 5)
    over = ps[(ps["work"] == 0) & (ps["script"] == 1)][0]
    assert (over["rivals"], over["rival_scripts"], over["contested_words"]) == (3, 1, 12)
    assert int(ps[(ps["work"] == 2)][0]["outcome"]) == abi.FS_SOURCE_ALONE
    assert [int(r["primary"]) for r in ws[ws["work"] == 3]] == [1, 0]   # a tie: the smaller script


def test_the_same_fan_words_in_the_neighbouring_work_are_no_rivals(path):
    ps, ws, ss, qs = check([[(0, 5, 6), (2, 5, 6)], [(1, 5, 6)], [(1, 5, 6), (2, 100, 6)]], 3)
    assert ps["rivals"].tolist() == [0, 1, 1, 0, 0]
    assert qs["works_both"].tolist() == [0, 1, 1] and qs["contests"].tolist() == [0, 0, 1]


def test_spans_that_end_at_the_largest_fan_index(path):
    a = [(0, TOP - 9, 10), (1, TOP - 5, 6)]
    b = [(0, TOP - 2, 3), (1, 0, 3), (1, TOP - 5, 3)]
    c = [(0, TOP - 12, 6), (0, TOP - 5, 6)]
    ps, ws, ss, qs = check([a, b, c], 2, min_words=3)
    first = ps[(ps["work"] == 0) & (ps["script"] == 0)][0]
    assert (first["fan_last"], first["rivals"], first["contested_words"], first["sole_words"]) == \
        (TOP, 3, 9, 1)
    assert ws["covered_words"].sum() == 10 + 6 + 3 + 3 + 3 + 6 + 6


def test_two_passages_of_one_script_that_touch(path):
    # a file with two records at one fan index: the word counts once in the union, twice in the
    # pair sums; with --min-words 1 a script has two passages at the very same word
    dup = (np.array([0] * 6, np.uint32), np.array([0, 1, 2, 2, 3, 4], np.uint32),
           np.array([0, 1, 2, 10, 11, 12], np.uint32), np.zeros(6))
    other, third = columns([(0, 0, 6)]), columns([(0, 2, 1)])
    for files, m in (([dup, other], 3), ([other, dup], 3), ([dup, other, third], 1),
                     ([third, dup, third], 1)):
        want = oracle(files, m)
        assert_equal(sources.find_sources(files, 1, m), want)
    want = oracle([dup, other], 3)
    assert want[0]["contested_words"].tolist() == [3, 5, 3] and want[3]["shared_words"][0] == 6


def test_a_file_without_records_and_a_work_in_one_file_only(path):
    ps, ws, ss, qs = check([[(0, 0, 6), (3, 0, 6)], [], [(3, 2, 6)]], 5)
    assert ss["passages"].tolist() == [2, 0, 1] and ss["works"].tolist() == [2, 0, 1]
    assert ws["work"].tolist() == [0, 3, 3] and ws["work_scripts"].tolist() == [1, 2, 2]
    assert qs["works_both"].tolist() == [0, 1, 0]
    # no run is a passage: tables of zeros
    ps, ws, ss, qs = check([[(0, 0, 5)], [(0, 0, 5)]], 1)
    assert len(ps) == 0 and len(ws) == 0 and not ss["works"].any() and qs["a"].tolist() == [0]


# ---- capacity, refusals, times --------------------------------------------------------------

def _call(L, files, n_works, out, cap_p, rows, cap_w, tabs, prs, n_p, n_w, min_words=6, K=None,
          n=None):
    arr = (abi.FsSourceCols * max(1, len(files)))()
    for s, (w, f, o, c) in enumerate(files):
        arr[s] = abi.FsSourceCols(abi.ptr(w, C.c_uint32), abi.ptr(f, C.c_uint32),
                                  abi.ptr(o, C.c_uint32), abi.ptr(c, C.c_double),
                                  len(w) if n is None else n)
    void = lambda a, cap: a.ctypes.data_as(C.c_void_p) if cap else None     # noqa: E731
    return L.fs_sources(0, arr, len(files) if K is None else K, n_works, min_words, 0,
                        void(out, cap_p), cap_p, C.byref(n_p), void(rows, cap_w), cap_w,
                        C.byref(n_w), tabs.ctypes.data_as(C.c_void_p),
                        prs.ctypes.data_as(C.c_void_p))


def test_capacity_zero_one_short_and_exact_for_both_arrays(path):
    files = [columns(s) for s in planted(3, 20, seed=5)]
    want = oracle(files)
    P, R = len(want[0]), len(want[1])
    assert P > 50 and R > 30
    L = _lib.load()
    n_p, n_w = C.c_uint64(0), C.c_uint64(0)
    for cap_p, cap_w in ((0, 0), (P - 1, R), (P, R - 1), (P, 0), (0, R)):
        out, rows = np.zeros(P, dtype=DTYPES[0]), np.zeros(R, dtype=DTYPES[1])
        tabs, prs = np.ones(3, dtype=DTYPES[2]), np.ones(3, dtype=DTYPES[3])
        rc = _call(L, files, 20, out, cap_p, rows, cap_w, tabs, prs, n_p, n_w)
        assert rc == abi.FS_E_CAPACITY and (n_p.value, n_w.value) == (P, R)
        assert_equal((want[0], want[1], tabs, prs), want)      # the fixed tables are complete
        assert not out.view(np.uint8).any() and not rows.view(np.uint8).any()   # untouched
    out, rows = np.zeros(P, dtype=DTYPES[0]), np.zeros(R, dtype=DTYPES[1])
    assert _call(L, files, 20, out, P, rows, R, tabs, prs, n_p, n_w) == abi.FS_OK
    assert_equal((out, rows, tabs, prs), want)


def test_refusals_and_times(path):
    spans = planted(3, 10, seed=6)
    files = [columns(s) for s in spans]

    def refused(fs, n_works=10, code=abi.FS_E_INVALID, **options):
        with pytest.raises(_lib.FsError) as e:
            sources.find_sources(fs, n_works, **options)
        assert e.value.code == code
    refused(files, n_works=int(files[2][0].max()))             # a work >= n_works
    refused(files, min_words=0)
    refused([])                                                # no files
    refused(files * 22, code=abi.FS_E_UNSUPPORTED)             # 66 files
    w, f, o, c = files[1]
    fan = f.copy()
    assert w[0] == w[1] and fan[0] < fan[1]
    fan[0], fan[1] = fan[1], fan[0]
    refused([files[0], (w, fan, o, c), files[2]])              # out of (work, fan_ix) order
    back = files[2][0].copy()
    assert back[-1] > 0
    back[-1] = 0
    refused([files[0], files[1], (back, files[2][1], files[2][2], files[2][3])])
    L = _lib.load()
    n_p, n_w = C.c_uint64(0), C.c_uint64(0)
    tabs, prs = np.zeros(3, dtype=DTYPES[2]), np.zeros(3, dtype=DTYPES[3])
    rc = _call(L, files, 10, tabs, 0, tabs, 0, tabs, prs, n_p, n_w, n=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                          # (refused before a record is read)
    check(spans, 10)                                           # and the same files are accepted
    ms = (C.c_double * 5)()
    assert L.fs_sources_times(ms) == abi.FS_OK
    assert min(ms[:4]) > 0 and ms[4] > max(ms[:4])


# ---- the randomised cross-check -------------------------------------------------------------

@pytest.mark.parametrize("seed,K,gap", [(1, 2, 0), (2, 2, 1), (3, 3, 0), (4, 6, 2), (5, 20, 0)])
def test_random_works_against_the_restatement(path, seed, K, gap):
    spans = planted(K, 40 if K < 10 else 12, seed=seed, anchors=5)
    rng = np.random.default_rng(100 + seed)
    files = []
    for s in spans:                                            # records left out: --max-gap joins
        w, f, o, c = columns(s)
        keep = rng.random(len(w)) > 0.04
        files.append((w[keep], f[keep], o[keep], c[keep]))
    want = oracle(files, 6, gap)
    got = sources.find_sources(files, 40, 6, gap)
    assert_equal(got, want)
    ps, ws, ss, qs = got
    assert len(ps) > 100 and qs["contests"].sum() > 20
    if K == 2:                                                 # no fan word twice in a file
        assert ps["contested_words"][ps["script"] == 0].sum() == qs["shared_words"][0]
        assert ps["contested_words"][ps["script"] == 1].sum() == qs["shared_words"][0]


# ---- the command ------------------------------------------------------------------------------

def inputs():
    return [os.path.join(GOLDEN, msg.input_name(s)) for s in msg.SCRIPTS]


def run_both(tmp_path, srcs, argv):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / reader)
        assert main(["sources"] + srcs + ["-o", prefix, "--reader", reader] + argv) == 0
        got[reader] = tuple(open(p, "rb").read() for p in sources.output_names(prefix))
    assert got["device"] == got["python"]
    return got["device"]


@pytest.mark.parametrize("case", msg.CASES, ids=[c[0] for c in msg.CASES])
def test_golden_cases_under_both_readers(tmp_path, path, case):
    out = run_both(tmp_path, inputs(), msg.arguments(case))
    texts = [open(p, newline="", encoding="utf-8").read() for p in inputs()]
    want = sr.sources_csv(texts, msg.NAMES, case[1], case[2])
    assert out == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(msg.golden_names(case[0]), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_the_default_names_and_an_off_grammar_file(tmp_path):
    import shutil
    srcs = []
    for s, name in zip(msg.SCRIPTS, msg.NAMES):
        os.makedirs(tmp_path / name)
        srcs.append(str(tmp_path / name / "match-6gram-20240101.csv"))
        shutil.copy(os.path.join(GOLDEN, msg.input_name(s)), srcs[-1])
    out = run_both(tmp_path, srcs, [])                  # the parent directories name the scripts
    for name, part in zip(msg.golden_names("default"), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name
    lines = open(srcs[1], "rb").read().split(b"\r\n")
    parts = lines[5].split(b",")
    parts[2] = b'fee"l"in'                       # a quote inside a field: csv.reader takes it
    lines[5] = b",".join(parts)
    with open(srcs[1], "wb") as fh:
        fh.write(b"\r\n".join(lines))
    with MatchFile(srcs[1]) as mf:
        assert mf.outside and mf.reason & abi.FS_MATCH_BAD_OPEN
    out = run_both(tmp_path, srcs, [])
    texts = [open(p, newline="", encoding="utf-8").read() for p in srcs]
    assert out == tuple(t.encode("utf-8") for t in sr.sources_csv(texts, msg.NAMES))
    assert b'fee""l""in' in out[0]
    with open(os.path.join(GOLDEN, msg.golden_names("default")[1]), "rb") as fh:
        assert out[1] == fh.read()               # (a fan word plays no part in the figures)


# ---- behind a several-script search ---------------------------------------------------------

def test_search_two_scripts_then_sources(tmp_path, monkeypatch, capsys):
    """20 works against two scripts that share one line of 12 words: the even works quote the
    shared line at fan word 10, every work a stretch of its own script at fan word 50."""
    words = synth.vocab_words()
    scripts = [synth.script_tokens(300, seed=400 + k) for k in range(2)]
    scripts[1][40:52] = scripts[0][100:112]
    sdir = tmp_path / "scripts"
    sdir.mkdir()
    paths = []
    for k, sc in enumerate(scripts):
        paths.append(str(sdir / ("script-%d.txt" % k)))
        with open(paths[-1], "w") as fh:
            fh.write(synth.script_markup(sc, words))
    fan = tmp_path / "fan"
    fan.mkdir()
    for i in range(20):
        tok = synth.script_tokens(90, seed=900 + i)
        if i % 2 == 0:
            tok[10:22] = scripts[0][100:112]
        own = scripts[(i // 2) % 2]
        tok[50:62] = own[200 + i:212 + i]
        (fan / synth.work_name(i)).write_text(" ".join(words[int(t)] for t in tok))
    monkeypatch.setenv("FANDOM_SEARCH_SYNTHETIC_VOCAB", "1")
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    try:
        assert main(["search", str(fan)] + paths + ["--synthetic-vocab", "--out-dir",
                                                    str(tmp_path / "multi")]) == 0
    finally:
        search.set_vocab(None)
    capsys.readouterr()
    dated = []
    for k in range(2):
        d = str(tmp_path / "multi" / ("script-%d" % k))
        every = set(glob.glob(os.path.join(d, "match-6gram-*.csv")))
        dated += sorted(every - set(glob.glob(os.path.join(d, "match-6gram-batch-*.csv"))))
    assert len(dated) == 2
    out = run_both(tmp_path, dated, [])
    import csv
    import io
    rows = list(csv.reader(io.StringIO(out[0].decode("utf-8"), newline="")))[1:]
    shared = [r for r in rows if int(r[2]) <= 21 and int(r[3]) >= 10]
    others = [r for r in rows if not (int(r[2]) <= 21 and int(r[3]) >= 10)]
    assert len(shared) == 20 and len(others) == 20
    assert {r[0] for r in rows} == {"script-0", "script-1"}
    assert all(r[10] == "1" and r[14] in ("won", "lost") and r[12] == "12" for r in shared)
    assert sorted(r[14] for r in shared) == ["lost"] * 10 + ["won"] * 10
    assert all(r[14] == "alone" and r[15] == "" for r in others)
    pairs = list(csv.reader(io.StringIO(out[3].decode("utf-8"), newline="")))[1:]
    assert pairs == [["script-0", "script-1", "10", "10", "120", "10", "0"]]
    texts = [open(p, newline="", encoding="utf-8").read() for p in dated]
    assert out == tuple(t.encode("utf-8")
                        for t in sr.sources_csv(texts, ["script-0", "script-1"]))
