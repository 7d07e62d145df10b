"""`ao3.py sources` without a GPU: the oracle's known answers worked by hand
(tests/sources_restated.py), the tie rules, the scripts' names, the parser, the C ABI's
declarations and the refusals that need no device, and the committed expected CSVs under the
product's table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, sources
from tests import sources_restated as sr
from tests.golden import make_sources_golden as msg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def span(work, fan, words, orig=0, exact=None):
    """The records (work, fan_ix, orig_ix, dist, comb) of one passage of `words` words, the
    first `exact` of them exact (default: all)."""
    exact = words if exact is None else exact
    return [(work, fan + k, orig + k, 0.0, 0.0 if k < exact else 0.5) for k in range(words)]


def by_span(got):
    return {(p["script"], p["fan_first"], p["fan_last"]): p for p in got["passages"]}


# ---- oracle known answers, worked by hand ------------------------------------------------

def test_the_hand_worked_chain():
    got = sr.sources([span(0, 0, 6), span(0, 4, 4), span(0, 7, 2)], min_words=2)
    a, b, c = got["passages"]
    assert [(p["script"], p["fan_first"], p["fan_last"]) for p in (a, b, c)] == \
        [(0, 0, 5), (1, 4, 7), (2, 7, 8)]
    assert (a["outcome"], a["rivals"], a["rival_scripts"], a["contested_words"], a["sole_words"],
            a["best_rival"]) == ("won", 1, 1, 2, 4, 1)
    assert (b["outcome"], b["rivals"], b["rival_scripts"], b["contested_words"], b["sole_words"],
            b["best_rival"]) == ("lost", 2, 2, 3, 1, 0)
    # C loses to B, which lost itself
    assert (c["outcome"], c["rivals"], c["rival_scripts"], c["contested_words"], c["sole_words"],
            c["best_rival"]) == ("lost", 1, 1, 1, 1, 1)
    assert (b["best_rival_words"], b["best_rival_fan_first"]) == (6, 0)
    pairs = {(p["a"], p["b"]): (p["contests"], p["shared_words"], p["a_wins"], p["works_both"])
             for p in got["pairs"]}
    assert pairs == {(0, 1): (1, 2, 1, 1), (1, 2): (1, 1, 1, 1), (0, 2): (0, 0, 0, 1)}
    assert [(p["a"], p["b"]) for p in got["pairs"]] == [(0, 1), (0, 2), (1, 2)]
    assert [(r["script"], r["covered_words"], r["primary"], r["work_scripts"])
            for r in got["works"]] == [(0, 6, 1, 3), (1, 4, 0, 3), (2, 2, 0, 3)]
    assert [(s["won"], s["lost"], s["alone"], s["primary_works"]) for s in got["scripts"]] == \
        [(1, 0, 0, 1), (0, 1, 0, 0), (0, 1, 0, 0)]


def test_the_tie_rules():
    # equal words: the exact words decide; equal both: the smaller script number
    got = by_span(sr.sources([span(0, 0, 6, exact=5), span(0, 0, 6)]))
    assert (got[(0, 0, 5)]["outcome"], got[(1, 0, 5)]["outcome"]) == ("lost", "won")
    got = by_span(sr.sources([span(0, 0, 6), span(0, 0, 6)]))
    assert (got[(0, 0, 5)]["outcome"], got[(1, 0, 5)]["outcome"]) == ("won", "lost")
    # more words beat more exact words
    got = by_span(sr.sources([span(0, 0, 7, exact=0), span(0, 0, 6)]))
    assert got[(0, 0, 6)]["outcome"] == "won"
    # the best rival: the key, then the smaller script, then the smaller fan start
    files = [span(0, 0, 20), span(0, 0, 6) + span(0, 10, 6), span(0, 12, 6)]
    best = by_span(sr.sources(files))[(0, 0, 19)]
    assert (best["rivals"], best["rival_scripts"], best["best_rival"],
            best["best_rival_fan_first"], best["outcome"]) == (3, 2, 1, 0, "won")
    # primary: the most covered words, a tie to the smaller script
    got = sr.sources([span(0, 0, 6), span(0, 20, 6), span(0, 40, 7)])
    assert [r["primary"] for r in got["works"]] == [0, 0, 1]
    got = sr.sources([span(0, 0, 6), span(0, 20, 6)])
    assert [r["primary"] for r in got["works"]] == [1, 0]
    assert [p["outcome"] for p in got["passages"]] == ["alone", "alone"]


def test_touching_is_a_contest_and_adjacent_is_not():
    touch = sr.sources([span(0, 0, 6), span(0, 5, 6)])
    assert [p["contested_words"] for p in touch["passages"]] == [1, 1]
    apart = sr.sources([span(0, 0, 6), span(0, 6, 6)])
    assert [p["rivals"] for p in apart["passages"]] == [0, 0]
    # the same fan words in the next work: no rival
    other = sr.sources([span(0, 0, 6), span(1, 0, 6)])
    assert [p["outcome"] for p in other["passages"]] == ["alone", "alone"]
    assert other["pairs"][0]["works_both"] == 0
    # a word two rivals cover counts once; the pair sums count it per pair
    both = sr.sources([span(0, 0, 10), span(0, 2, 6), span(0, 4, 6)])
    assert both["passages"][0]["contested_words"] == 8
    assert [p["shared_words"] for p in both["pairs"]] == [6, 6, 4]
    # one file with two records at one fan index: two passages of one script that touch
    dup = [(0, k, k, 0.0, 0.0) for k in range(3)] + [(0, 2 + k, 10 + k, 0.0, 0.0) for k in range(3)]
    got = sr.sources([dup, span(0, 0, 6)], min_words=3)
    assert [(p["script"], p["fan_first"], p["fan_last"]) for p in got["passages"]] == \
        [(0, 0, 2), (1, 0, 5), (0, 2, 4)]
    assert got["passages"][1]["contested_words"] == 5 and got["pairs"][0]["shared_words"] == 6


def test_spans_at_the_end_of_the_index_range():
    top = (1 << 32) - 1
    got = sr.sources([span(0, top - 5, 6), span(0, top - 2, 3)], min_words=3)
    assert [(p["contested_words"], p["sole_words"]) for p in got["passages"]] == [(3, 3), (3, 0)]
    assert got["passages"][0]["fan_last"] == top


# ---- product side that needs no GPU ----------------------------------------------------

def test_script_names_and_their_errors():
    assert sources.script_names(["out/hope/m.csv", "out/empire/m.csv"]) == ["hope", "empire"]
    assert sources.script_names(["out/hope.csv", "out/empire.csv"]) == ["hope", "empire"]
    assert sources.script_names(["x/a.csv", "x/b", "y/c.csv"]) == ["a", "b", "c"]
    assert sources.script_names(["x/a.csv", "x/b.csv"], "one,two") == ["one", "two"]
    assert sources.script_names(["x/a.csv", "x/a.csv"], ["p", "q"]) == ["p", "q"]
    with pytest.raises(ValueError, match="at least two"):
        sources.script_names(["x/a.csv"])
    with pytest.raises(ValueError, match="3 names for 2 files"):
        sources.script_names(["x/a.csv", "x/b.csv"], "p,q,r")
    with pytest.raises(ValueError, match="both named 'a'"):
        sources.script_names(["x/a.csv", "x/a"])
    with pytest.raises(ValueError, match="both named 'p'"):
        sources.script_names(["x/a.csv", "y/b.csv"], "p,p")


def test_parser_defaults_and_output_names():
    args = cli.build_parser().parse_args(["sources", "a/m.csv", "b/m.csv", "-o", "out/x"])
    assert args.func.__name__ == "_sources"
    assert (args.matches, args.output, args.names, args.min_words, args.max_gap, args.device,
            args.reader) == (["a/m.csv", "b/m.csv"], "out/x", None, 6, 0, 0, None)
    assert sources.output_names("out/x") == ("out/x-sources.csv", "out/x-sources-works.csv",
                                             "out/x-sources-scripts.csv",
                                             "out/x-sources-pairs.csv")
    args = cli.build_parser().parse_args(
        ["sources", "a.csv", "b.csv", "c.csv", "-o", "p", "--names", "x,y,z", "--min-words", "3",
         "--max-gap", "2", "--device", "1", "--reader", "python"])
    assert (len(args.matches), args.names, args.min_words, args.max_gap, args.device,
            args.reader) == (3, "x,y,z", 3, 2, 1, "python")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["sources", "a.csv", "b.csv"])        # -o is required
    assert (sources.PASSAGE_FIELDS, sources.WORK_FIELDS, sources.SCRIPT_FIELDS,
            sources.PAIR_FIELDS) == (sr.PASSAGE_FIELDS, sr.WORK_FIELDS, sr.SCRIPT_FIELDS,
                                     sr.PAIR_FIELDS)
    assert sources.OUTCOMES == (sr.ALONE, sr.WON, sr.LOST)
    assert "sources" in cli.build_parser().format_help() and "sources" in cli.__doc__


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--max-gap", "-1"], ["--names", "a"],
                                 ["--names", "a,a"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["sources", str(tmp_path / "a.csv"), str(tmp_path / "b.csv"), "-o",
                  str(tmp_path / "x")] + bad)
    assert str(e.value.code).startswith("ao3.py sources: error: ")


def test_one_file_exits_with_an_error_line(tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["sources", str(tmp_path / "a.csv"), "-o", str(tmp_path / "x")])
    assert str(e.value.code).startswith("ao3.py sources: error: sources joins")


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_sources", "fs_sources_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.SOURCES_MS_NAMES == ("passages", "contest", "union", "rollups", "total")
    assert (abi.FS_SOURCES_MAX_FILES, abi.FS_SOURCES_MAX_BYTES) == (64, 1 << 30)
    assert "#define FS_SOURCES_MAX_FILES 64u" in text
    assert "#define FS_SOURCES_MAX_BYTES (1ull << 30)" in text
    for k, name in enumerate(("ALONE", "WON", "LOST")):
        assert "#define FS_SOURCE_%s %du" % (name, k) in text
        assert getattr(abi, "FS_SOURCE_" + name) == k


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_source_passage", "SOURCE_PASSAGE_DTYPE", sr.PASSAGE_KEYS, 80),
    ("fs_source_work", "SOURCE_WORK_DTYPE", sr.WORK_KEYS, 56),
    ("fs_source_script", "SOURCE_SCRIPT_DTYPE", sr.SCRIPT_KEYS, 48),
    ("fs_source_pair", "SOURCE_PAIR_DTYPE", sr.PAIR_KEYS, 48)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for bits, names in re.findall(r"uint(32|64)_t\s+([^;]+);", body):
        for n in names.split(","):
            assert at % (int(bits) // 8) == 0
            fields.append((n.strip(), at, int(bits) // 8))
            at += int(bits) // 8
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_the_columns_struct_matches_the_header():
    assert C.sizeof(abi.FsSourceCols) == 40
    assert [(n, getattr(abi.FsSourceCols, n).offset) for n, _ in abi.FsSourceCols._fields_] == \
        [("work", 0), ("fan_ix", 8), ("orig_ix", 16), ("comb", 24), ("n", 32)]


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    d = np.zeros(4, dtype=np.float64)
    u32, f64 = abi.ptr(z, C.c_uint32), abi.ptr(d, C.c_double)
    passages = np.ones(2, dtype=abi.SOURCE_PASSAGE_DTYPE)
    works = np.ones(2, dtype=abi.SOURCE_WORK_DTYPE)
    scripts = np.ones(64, dtype=abi.SOURCE_SCRIPT_DTYPE)
    pairs = np.ones(2016, dtype=abi.SOURCE_PAIR_DTYPE)
    n_p, n_w = C.c_uint64(7), C.c_uint64(7)
    void = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731

    def call(K=2, n=1, n_works=1, min_words=1, cols=True, files=True, out=void(passages),
             rows=void(works), n_out=C.byref(n_p), tabs=void(scripts), prs=void(pairs)):
        arr = (abi.FsSourceCols * max(1, K))()
        for s in range(K):
            arr[s] = abi.FsSourceCols(u32 if cols else None, u32, u32, f64, n)
        return L.fs_sources(0, arr if files else None, K, n_works, min_words, 0, out, 2, n_out,
                            rows, 2, C.byref(n_w), tabs, prs)
    assert call(K=65) == abi.FS_E_UNSUPPORTED
    assert call(n=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(K=65, min_words=0) == abi.FS_E_UNSUPPORTED       # before anything is read
    assert call(n_works=1 << 31) == abi.FS_E_UNSUPPORTED         # 12 bytes per work: over the cap
    assert call(n=(abi.FS_SOURCES_MAX_BYTES // 28) + 1) == abi.FS_E_UNSUPPORTED
    assert call(K=0) == abi.FS_E_INVALID
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(files=False) == abi.FS_E_INVALID
    assert call(cols=False) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID                    # a capacity without a buffer
    assert call(rows=None) == abi.FS_E_INVALID
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(tabs=None) == abi.FS_E_INVALID
    assert call(prs=None) == abi.FS_E_INVALID
    assert (n_p.value, n_w.value) == (7, 7)
    assert (scripts["works"] == 1).all() and (pairs["a"] == 1).all()   # nothing written
    # no records at all: tables of zeros, no device work
    assert call(K=3, n=0, cols=False) == abi.FS_OK
    assert (n_p.value, n_w.value) == (0, 0)
    assert [tuple(r) for r in scripts[:3].tolist()] == [(0,) * 9] * 3
    assert [tuple(r)[:3] for r in pairs[:3].tolist()] == [(0, 1, 0), (0, 2, 0), (1, 2, 0)]
    assert (scripts["works"][3:] == 1).all() and (passages["script"] == 1).all()
    assert call(K=1, n=0, prs=None) == abi.FS_OK                 # one file has no pairs
    assert L.fs_sources_times(None) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        sources.find_sources([(z, z, z[:3], d)], 1)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(files, n_works, min_words=6, max_gap=0, device=0):
    recs = [list(zip(*(np.asarray(c).tolist() for c in (work, fan, orig, comb, comb))))
            for work, fan, orig, comb in files]
    for r in recs:
        assert all(t[0] < n_works for t in r)
    tabs = sr.as_tuples(sr.sources(recs, min_words, max_gap))
    return tuple(np.array(t, dtype=dt) for t, dt in zip(tabs, (
        abi.SOURCE_PASSAGE_DTYPE, abi.SOURCE_WORK_DTYPE, abi.SOURCE_SCRIPT_DTYPE,
        abi.SOURCE_PAIR_DTYPE)))


def csv_text(head, part):
    buf = io.StringIO(newline="")
    csv.writer(buf).writerows([head] + part)
    return buf.getvalue().encode("utf-8")


def test_the_golden_generator_reproduces_its_committed_files():
    made = msg.build()
    assert set(made) == ({msg.input_name(s) for s in msg.SCRIPTS}
                         | {n for c in msg.CASES for n in msg.golden_names(c[0])})
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name
        assert len(text.encode("utf-8")) < 16 << 10


@pytest.mark.parametrize("case", msg.CASES, ids=[c[0] for c in msg.CASES])
def test_the_tables_under_the_oracle_give_the_goldens(case):
    files = [sources.open_file(os.path.join(GOLDEN, msg.input_name(s)), "python")
             for s in msg.SCRIPTS]
    body = sources.tables(files, msg.NAMES, case[1], case[2], find=oracle_find)
    heads = (sources.PASSAGE_FIELDS, sources.WORK_FIELDS, sources.SCRIPT_FIELDS,
             sources.PAIR_FIELDS)
    for name, head, part in zip(msg.golden_names(case[0]), heads, body):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert csv_text(head, part) == fh.read(), name


def test_the_shared_numbering_and_the_second_sort():
    files = [sources.open_file(os.path.join(GOLDEN, msg.input_name(s)), "python")
             for s in msg.SCRIPTS]
    names, cols = sources.shared_order(files)
    assert names == ["a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt", "g.txt", "h.txt",
                     "i.txt", "k.txt", "l.txt", "m.txt", "j.txt"]
    for (order, work, fan, orig, comb), f in zip(cols, files):
        assert sorted(order.tolist()) == list(range(len(f.rows)))
        keys = list(zip(work.tolist(), fan.tolist()))
        assert keys == sorted(keys)
        assert [f.rows[i][0] for i in order.tolist()] == [names[w] for w in work.tolist()]
    # empire lists g before f, jedi has j in its middle: neither file's own order is the shared one
    assert [f.names == [n for n in names if n in f.names] for f in files] == [True, False, False]


def test_the_golden_inputs_hold_what_their_generator_says():
    from tests import passages_restated as pr
    made = msg.build()
    rows = [pr.read_rows(made[msg.input_name(s)]) for s in msg.SCRIPTS]
    assert len({r[0] for part in rows for r in part}) == 13
    assert all(40 <= len(part) <= 120 for part in rows)
    assert any("/" in r[0] for r in rows[0]) and any("," in r[8] for r in rows[0])
    assert "e.txt" not in {r[0] for r in rows[1]}                    # missing from one file
    assert all("j.txt" not in {r[0] for r in part} for part in rows[:2])

    def table(case, kind):
        text = made[msg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    passages = table("default", 0)
    of = {(r[0], r[1], r[2]): r for r in passages}
    assert [of[(s, "a.txt", "10")][14] for s in msg.NAMES] == ["won", "lost", "lost"]   # all share
    assert (of[("hope", "b.txt", "5")][14], of[("empire", "b.txt", "5")][14]) == ("lost", "won")
    assert (of[("hope", "b.txt", "5")][7], of[("empire", "b.txt", "5")][7]) == ("6", "7")
    assert of[("hope", "dir/c.txt", "3")][14:18] == ["alone", "", "", ""]
    chain = [of[("hope", "d.txt", "0")], of[("empire", "d.txt", "10")], of[("jedi", "d.txt", "17")]]
    assert [(r[14], r[10], r[11], r[12], r[13], r[15]) for r in chain] == [
        ("won", "1", "1", "2", "10", "empire"), ("lost", "2", "2", "3", "5", "hope"),
        ("lost", "1", "1", "1", "5", "empire")]
    assert [r[14] for r in passages if r[1] == "l.txt"] == ["alone", "alone"]       # adjacent
    assert [r[12] for r in passages if r[1] == "m.txt"] == ["1", "1"]               # touching
    assert passages[-1][1] == "j.txt"                                               # numbered last
    assert ("jedi", "h.txt", "6") not in of
    gap = {(r[0], r[1], r[2]): r for r in table("gap1", 0)}
    assert gap[("jedi", "h.txt", "6")][6:8] == ["6", "6"] and gap[("jedi", "h.txt", "6")][14] == "lost"
    works = table("default", 1)
    assert [r[10] for r in works if r[0] == "i.txt"] == ["1", "0", "0"]
    assert table("default", 3) == [["hope", "empire", "8", "9", "57", "8", "1"],
                                   ["hope", "jedi", "6", "3", "15", "3", "0"],
                                   ["empire", "jedi", "3", "3", "15", "3", "0"]]
