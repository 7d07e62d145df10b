"""`ao3.py pairs` without a GPU: the oracle's known answers, the parser, the C ABI's
declarations and the committed expected CSVs."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import pairs_restated as pp
from tests import passages_restated as pr
from tests.golden import make_pairs_golden as mpg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _diag(work, fan0, orig0, n):
    return [(work, fan0 + k, orig0 + k) for k in range(n)]


def _work(covered=0, partners=0, best=pp.NONE, best_shared=0):
    return dict(covered=covered, partners=partners, best=best, best_shared=best_shared)


def _pair(a, b, shared, first, last, run_first, run_words):
    return dict(a=a, b=b, shared=shared, first=first, last=last, run_first=run_first,
                run_words=run_words)


# ---- oracle known answers -------------------------------------------------------------

def test_identical_coverage_shares_all_of_it():
    works, pairs = pp.pairs(_diag(0, 5, 10, 8) + _diag(1, 0, 10, 8), 2, 20)
    assert works == [_work(8, 1, 1, 8), _work(8, 1, 0, 8)]
    assert pairs == [_pair(0, 1, 8, 10, 17, 10, 8)]


def test_disjoint_coverage_makes_no_pair():
    works, pairs = pp.pairs(_diag(0, 0, 0, 6) + _diag(1, 0, 6, 6) + _diag(2, 0, 30, 3), 3, 40,
                            min_shared=1)
    assert pairs == []
    assert works == [_work(6), _work(6), _work()]          # (work 2 has no passage)


def test_a_bridged_word_is_shared_under_the_gap_only():
    # work 0 steps over script word 3; work 1 covers 3..8
    recs = [(0, f, f) for f in (0, 1, 2, 4, 5, 6)] + _diag(1, 0, 3, 6)
    works, pairs = pp.pairs(recs, 2, 9, min_words=3, max_gap=1, min_shared=1)
    assert works[0]["covered"] == 7 and pairs == [_pair(0, 1, 4, 3, 6, 3, 4)]
    # without the gap work 0 has the passages 0..2 and 4..6: word 3 is not covered
    works, pairs = pp.pairs(recs, 2, 9, min_words=3, max_gap=0, min_shared=1)
    assert works[0]["covered"] == 6 and pairs == [_pair(0, 1, 3, 4, 6, 4, 3)]


def test_a_work_repeating_a_line_counts_it_once():
    recs = _diag(0, 0, 10, 6) + _diag(0, 20, 10, 6) + _diag(1, 0, 10, 6)
    works, pairs = pp.pairs(recs, 2, 16)
    assert works == [_work(6, 1, 1, 6), _work(6, 1, 0, 6)]
    assert pairs == [_pair(0, 1, 6, 10, 15, 10, 6)]


def test_the_longest_run_is_the_first_among_equals():
    # shared words 0..2, 10..12 and 20..21
    recs = (_diag(0, 0, 0, 3) + _diag(0, 10, 10, 3) + _diag(0, 20, 20, 2) + _diag(1, 0, 0, 30))
    works, pairs = pp.pairs(recs, 2, 30, min_words=2, min_shared=1)
    assert pairs == [_pair(0, 1, 8, 0, 21, 0, 3)]
    assert pp.longest_run({5, 6, 9, 10, 11, 20, 21, 22}) == (9, 3)
    assert pp.longest_run({7}) == (7, 1)


def test_the_best_partner_is_the_smaller_work_on_a_tie():
    recs = _diag(0, 0, 0, 6) + _diag(1, 0, 0, 12) + _diag(2, 0, 6, 6) + _diag(3, 0, 0, 6)
    works, pairs = pp.pairs(recs, 4, 12)
    assert [(p["a"], p["b"], p["shared"]) for p in pairs] == [(0, 1, 6), (0, 3, 6), (1, 2, 6),
                                                              (1, 3, 6)]
    assert works == [_work(6, 2, 1, 6), _work(12, 3, 0, 6), _work(6, 1, 1, 6),
                     _work(6, 2, 0, 6)]


def test_min_shared_above_every_pair_leaves_none():
    recs = _diag(0, 0, 0, 8) + _diag(1, 0, 2, 8) + _diag(2, 0, 4, 8)
    works, pairs = pp.pairs(recs, 3, 12, min_shared=1)
    assert max(p["shared"] for p in pairs) == 6 and len(pairs) == 3
    works, pairs = pp.pairs(recs, 3, 12, min_shared=7)
    assert pairs == [] and works == [_work(8), _work(8), _work(8)]
    works, pairs = pp.pairs(recs, 3, 12, min_shared=6)
    assert [(p["a"], p["b"]) for p in pairs] == [(0, 1), (1, 2)]
    assert works == [_work(8, 1, 1, 6), _work(8, 2, 0, 6), _work(8, 1, 1, 6)]


def test_refusals_and_no_records():
    ok = _diag(0, 0, 0, 3)
    for kw in (dict(min_words=0), dict(min_shared=0), dict(n_works=0), dict(n_script=2)):
        args = dict(n_works=1, n_script=3, min_words=1, min_shared=1)
        args.update(kw)
        with pytest.raises(ValueError):
            pp.pairs(ok, **args)
    with pytest.raises(ValueError):
        pp.pairs([(0, 1, 0), (0, 0, 1)], 1, 3)
    assert pp.pairs([], 2, 2) == ([_work(), _work()], [])


def _row(name, fan, orig, scene="1", char="ANNA", word=None):
    return [name, fan, "f%d" % fan, 1, orig, word or "W%d" % orig, 2, char, scene, "0.0", 7, "0.0"]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_two_files():
    rows = ([_row("b.txt", f, f + 10, scene="3", char="BOB") for f in (0, 1, 2, 4, 5, 6)] +
            [_row("a.txt", f, f + 11, scene="3", char="BOB") for f in (0, 1, 3, 4, 5, 6)] +
            [_row("c.txt", f, f + 40) for f in range(6)] + [_row("d.txt", 0, 12, "3", "BOB")])
    pairs, works = pp.pairs_csv(_match_csv(rows), 6, 1, 1)
    # b covers 10..16, a covers 11..17; both bridge word 13, which no record names
    assert pairs.split("\r\n")[1:] == [
        "b.txt,a.txt,7,7,6,11,16,11,6,BOB,3,W11 W12 [?] W14 W15 W16", ""]
    assert works.split("\r\n")[1:] == ["b.txt,7,1,a.txt,6", "a.txt,7,1,b.txt,6", "c.txt,6,0,,0", ""]
    assert pp.pairs_csv(_match_csv(rows, header=False), 6, 1, 1) == (pairs, works)
    assert pp.pairs_csv(_match_csv(rows), 6, 1, 7)[0] == ",".join(pp.PAIR_FIELDS) + "\r\n"


def test_a_script_word_with_two_labels_is_an_error(tmp_path):
    rows = [_row("a.txt", 0, 5), _row("a.txt", 1, 6), _row("b.txt", 0, 5, scene="4")]
    with pytest.raises(ValueError):
        pp.pairs_csv(_match_csv(rows))
    path = tmp_path / "two.csv"
    path.write_text(_match_csv(rows), newline="")
    with pytest.raises(SystemExit) as e:                  # (the labels are read before the GPU)
        cli.main(["pairs", str(path), "--reader", "python"])
    assert str(e.value.code).startswith("ao3.py pairs: error: script word 5 ")


def test_empty_input():
    pairs, works = pp.pairs_csv("")
    assert pairs == ",".join(pp.PAIR_FIELDS) + "\r\n"
    assert works == ",".join(pp.WORK_FIELDS) + "\r\n"


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import pairs
    args = cli.build_parser().parse_args(["pairs", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_pairs"
    assert (args.output, args.min_words, args.max_gap, args.min_shared, args.device,
            args.reader) == (None, 6, 0, 6, 0, None)
    assert pairs.output_names(args.matches) == ("runs/match-6gram-20240101-pairs.csv",
                                                "runs/match-6gram-20240101-pairs-works.csv")
    assert pairs.output_names("batch", None)[0] == "batch-pairs.csv"
    assert pairs.output_names("m.csv", "out/x")[1] == "out/x-pairs-works.csv"
    args = cli.build_parser().parse_args(["pairs", "m.csv", "-o", "p", "--min-words", "3",
                                          "--max-gap", "2", "--min-shared", "4", "--device", "1"])
    assert (args.output, args.min_words, args.max_gap, args.min_shared, args.device) == \
        ("p", 3, 2, 4, 1)
    assert pairs.PAIR_FIELDS == pp.PAIR_FIELDS
    assert pairs.WORK_FIELDS == pp.WORK_FIELDS
    assert pairs.UNKNOWN_WORD == pp.UNKNOWN_WORD == "[?]"


@pytest.mark.parametrize("bad", [["--min-shared", "0"], ["--min-words", "0"], ["--max-gap", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["pairs", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py pairs: error: ")


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_pairs_entry_points():
    for name in ("fs_pairs", "fs_pairs_rows", "fs_pairs_times"):
        assert name in _declared_functions()
        assert name in _lib.SYMBOLS
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    assert hasattr(lib, "fs_pairs") and hasattr(lib, "fs_pairs_rows")


@pytest.mark.parametrize("struct,dtype,size,keys",
                         [("fs_pair_work", "PAIR_WORK_DTYPE", 16, pp.WORK_KEYS),
                          ("fs_pair", "PAIR_DTYPE", 32, pp.PAIR_KEYS + ["reserved"])])
def test_dtypes_match_the_header(struct, dtype, size, keys):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for names in re.findall(r"uint32_t\s+([^;]+);", body):
        fields += [n.strip() for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == 4 * len(fields)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, 4 * k) for k, n in enumerate(fields)]
    assert list(dt.names) == keys
    assert re.search(r"#define FS_PAIRS_MAX_BYTES \(1u << 30\)", text)
    assert abi.FS_PAIRS_MAX_BYTES == 1 << 30


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    works = np.ones(2, dtype=abi.PAIR_WORK_DTYPE)
    u32 = abi.ptr(z, C.c_uint32)
    w = works.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, min_words=6, min_shared=6, works=w, cap=0, n_pairs=C.byref(n)):
        return L.fs_pairs(0, u32, u32, u32, n_rows, 2, n_script, min_words, 0, min_shared, works,
                          None, cap, n_pairs)
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_shared=0) == abi.FS_E_INVALID
    assert b"at least 1" in L.fs_last_error()
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(works=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                     # a capacity without a buffer
    assert call(n_pairs=None) == abi.FS_E_INVALID
    # no records: works without coverage, without device work
    assert call(n_rows=0) == abi.FS_OK and n.value == 0
    assert works.tolist() == [(0, 0, pp.NONE, 0)] * 2
    assert L.fs_pairs_rows(None, None, 0, 0, 6, 0, 6, None, None, 0,
                           C.byref(n)) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_cases_are_those_of_the_issue():
    from tests.golden import make_quotes_golden as mqg
    assert len(mpg.CASES) == 14 and {c[4] for c in mpg.CASES} == {1, 6}
    assert {c[0] for c in mpg.CASES} == set(mqg.NAMES)
    assert {c[:4] for c in mpg.CASES} == {c[:4] for c in mqg.CASES}


# kept pairs of every case at --min-shared 1 and 6
KEPT = {"synthetic_small": (2, 1), "synthetic_n4": (3, 3), "matrix_spans_a": (3, 3),
        "matrix_spans_b": (13, 1), "matrix_spans_c": (3, 1)}


@pytest.mark.parametrize("case,src,m,g,s", mpg.CASES)
def test_golden_files_are_the_oracle_output(case, src, m, g, s):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    got = pp.pairs_csv(text, m, g, s)
    for name, part in zip(mpg.golden_names(case, m, g, s), got):
        with open(os.path.join(gold, name), newline="", encoding="utf-8") as fh:
            want = fh.read()
        assert part == want, name
        assert want.count("\r\n") > 1                   # no file is empty of pairs or works
    assert got[0].count("\r\n") - 1 == KEPT[case][s == 6]
