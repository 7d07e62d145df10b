"""`ao3.py passages` without a GPU: the oracle's known answers, the parser, the C ABI's
declarations and the committed expected passage CSVs."""

import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import passages_restated as pr
from tests.golden import make_passages_golden as mpg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _rec(work, fan, orig, dist=0.0, comb=0.0):
    return (work, fan, orig, dist, comb)


def _diag(work, fan0, orig0, n, dist=0.0, comb=0.0):
    return [_rec(work, fan0 + k, orig0 + k, dist, comb) for k in range(n)]


def _spans(ps):
    return [(p["first"], p["n_words"]) for p in ps]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- oracle known answers -------------------------------------------------------------

def test_diagonal_run_is_one_passage():
    recs = _diag(0, 5, 100, 8, dist=0.25, comb=0.5)
    assert pr.passages(recs, 6) == [dict(first=0, n_words=8, n_exact=0, dist_sum=2.0,
                                         dist_max=0.25, comb_sum=4.0, comb_max=0.5)]


def test_script_jump_and_fan_gap_break_a_run():
    jump = _diag(0, 0, 10, 6) + _diag(0, 6, 30, 6)          # fan contiguous, script jumps
    assert _spans(pr.passages(jump, 6)) == [(0, 6), (6, 6)]
    gap = _diag(0, 0, 10, 6) + _diag(0, 7, 17, 6)           # one fan and script word missing
    assert _spans(pr.passages(gap, 6)) == [(0, 6), (6, 6)]
    back = _diag(0, 0, 10, 6) + _diag(0, 6, 15, 6)          # script steps back
    assert _spans(pr.passages(back, 6)) == [(0, 6), (6, 6)]


@pytest.mark.parametrize("gap", [1, 2])
def test_max_gap_bridges_missing_words(gap):
    recs = _diag(0, 0, 10, 4) + _diag(0, 4 + gap, 14 + gap, 4)
    assert _spans(pr.passages(recs, 6, max_gap=0)) == []
    assert _spans(pr.passages(recs, 6, max_gap=gap)) == [(0, 8)]
    assert _spans(pr.passages(recs, 6, max_gap=gap - 1)) == []
    # a fan gap of G with a script step of G + 2 stays broken
    skew = _diag(0, 0, 10, 4) + _diag(0, 4 + gap, 15 + gap, 4)
    assert _spans(pr.passages(skew, 6, max_gap=gap)) == []


def test_repeated_fan_index_ends_a_run():
    recs = _diag(0, 0, 10, 6) + [_rec(0, 5, 16)] + _diag(0, 6, 17, 6)
    assert _spans(pr.passages(recs, 6)) == [(0, 6), (6, 7)]     # the repeat starts a run
    recs = _diag(0, 0, 10, 6) + [_rec(0, 5, 40)] + _diag(0, 6, 17, 6)
    assert _spans(pr.passages(recs, 6)) == [(0, 6), (7, 6)]
    assert _spans(pr.passages(recs, 1)) == [(0, 6), (6, 1), (7, 6)]


def test_no_run_across_a_work_boundary():
    recs = _diag(0, 0, 10, 4) + _diag(1, 4, 14, 4)
    assert _spans(pr.passages(recs, 4)) == [(0, 4), (4, 4)]
    assert _spans(pr.passages(recs, 5)) == []


@pytest.mark.parametrize("m", range(1, 13))
def test_min_words(m):
    recs = _diag(0, 0, 0, 3) + _diag(0, 10, 50, 7) + _diag(1, 0, 0, 12)
    want = [(a, n) for a, n in [(0, 3), (3, 7), (10, 12)] if n >= m]
    assert _spans(pr.passages(recs, m)) == want


@pytest.mark.parametrize("at", range(6))
def test_nan_and_negative_zero_at_every_position(at):
    d = [0.5, 0.25, 0.125, 0.0625, 0.75, 0.375]
    c = list(d)
    d[at] = NAN
    c[at] = -0.0
    recs = [_rec(0, k, k, d[k], c[k]) for k in range(6)]
    (p,) = pr.passages(recs, 6)
    assert math.isnan(p["dist_sum"])
    assert p["dist_max"] == max(v for v in d if not math.isnan(v))
    assert p["n_exact"] == 1
    assert p["comb_max"] == max(c)
    s = 0.0
    for v in c:
        s += v
    assert _bits(p["comb_sum"]) == _bits(s)


def test_all_nan_and_signed_zero_ties():
    recs = [_rec(0, k, k, NAN, 0.0 if k == 0 else -0.0) for k in range(6)]
    (p,) = pr.passages(recs, 6)
    assert math.isnan(p["dist_max"]) and math.isnan(p["dist_sum"])
    assert _bits(p["comb_max"]) == _bits(0.0)          # the earlier 0.0 wins the tie
    assert _bits(p["comb_sum"]) == _bits(0.0)          # +0.0 + -0.0 = +0.0
    assert p["n_exact"] == 6
    recs = [_rec(0, k, k, 1.0, -0.0 if k == 0 else 0.0) for k in range(6)]
    (p,) = pr.passages(recs, 6)
    assert _bits(p["comb_max"]) == _bits(-0.0)
    assert _bits(p["comb_sum"]) == _bits(0.0)          # the sum starts at +0.0


def test_empty_input():
    assert pr.passages([], 6) == []
    assert pr.passages_csv("", 6) == "\r\n".join([",".join(pr.PASSAGE_FIELDS), ""])


def test_unsorted_records_are_refused():
    with pytest.raises(ValueError):
        pr.passages([_rec(0, 5, 5), _rec(0, 4, 6)], 1)
    with pytest.raises(ValueError):
        pr.passages([_rec(1, 0, 5), _rec(0, 1, 6)], 1)


def _match_csv(rows, header):
    import csv
    import io
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def _row(name, fan, word, orig, dist="0.0", comb="0.0"):
    return [name, fan, word, 1, orig, "W%d" % orig, 2, "ANNA", 3, dist, 7, comb]


def test_header_and_no_header_inputs_agree():
    rows = [_row("b.txt", 7 + k, "w%d" % k, 40 + k) for k in range(6)] + \
           [_row("a.txt", k, "v%d" % k, 10 + k) for k in range(6)]
    got = pr.passages_csv(_match_csv(rows, True), 6)
    assert got == pr.passages_csv(_match_csv(rows, False), 6)
    lines = got.split("\r\n")
    assert lines[1].startswith("b.txt,7,12,40,45,6,6,ANNA,3,0.0,0.0,0.0,0.0,w0 w1")
    assert lines[2].startswith("a.txt,0,5,10,15,6,6,ANNA,3,")


def test_sort_is_stable_by_first_appearance_of_the_work():
    rows = [_row("z.txt", 5 - k, "x", 15 - k) for k in range(6)]
    got = pr.passages_csv(_match_csv(rows, True), 6).split("\r\n")
    assert got[1].startswith("z.txt,0,5,10,15,6,")


def test_fan_words_that_look_like_missing_values_survive():
    words = ["nan", "null", "NA", "", "N/A", "None"]
    rows = [_row("a.txt", k, words[k], 10 + k, dist="", comb="") for k in range(6)]
    got = pr.passages_csv(_match_csv(rows, False), 6).split("\r\n")[1]
    assert got.endswith(",nan,nan,nan,nan,nan null NA  N/A None,W10 W11 W12 W13 W14 W15")
    assert ",6,0,ANNA," in got                             # no exact words: NaN is never <= 0


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_name():
    from fandom_search_amd import passages
    args = cli.build_parser().parse_args(["passages", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_passages"
    assert (args.output, args.min_words, args.max_gap, args.device) == (None, 6, 0, 0)
    assert passages.output_name(args.matches) == "runs/match-6gram-20240101-passages.csv"
    assert passages.output_name("batch") == "batch-passages.csv"
    args = cli.build_parser().parse_args(["passages", "m.csv", "-o", "p.csv", "--min-words", "3",
                                          "--max-gap", "2", "--device", "1"])
    assert (args.output, args.min_words, args.max_gap, args.device) == ("p.csv", 3, 2, 1)
    assert passages.PASSAGE_FIELDS == pr.PASSAGE_FIELDS


def test_host_sort_matches_the_oracle_order():
    from fandom_search_amd import passages
    rows = [_row("b.txt", 3, "x", 1), _row("a.txt", 2, "y", 2), _row("b.txt", 1, "z", 3),
            _row("b.txt", 3, "q", 4), _row("a.txt", 0, "r", 5)]
    order, work, fan, orig, dist, comb = passages.sort_records(
        [[str(v) for v in r] for r in rows])
    assert list(order) == [2, 0, 3, 4, 1]
    assert list(work) == [0, 0, 0, 1, 1] and list(fan) == [1, 3, 3, 0, 2]


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_passage_entry_points():
    for name in ("fs_passages", "fs_passages_rows"):
        assert name in _declared_functions()
        assert name in _lib.SYMBOLS
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    assert hasattr(lib, "fs_passages") and hasattr(lib, "fs_passages_rows")


def test_passage_dtype_matches_the_header():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct fs_passage \{(.*?)\} fs_passage;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    size = {"uint64_t": 8, "uint32_t": 4, "double": 8}
    off, want = 0, []
    for n, t in fields:
        off = (off + size[t] - 1) // size[t] * size[t]
        want.append((n, off))
        off += size[t]
    assert abi.PASSAGE_DTYPE.itemsize == 48 == off
    assert [(n, abi.PASSAGE_DTYPE.fields[n][1]) for n in abi.PASSAGE_DTYPE.names] == want


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(1, dtype=np.uint32)
    d = np.zeros(1, dtype=np.float64)
    u32 = abi.ptr(z, C.c_uint32)
    f64 = abi.ptr(d, C.c_double)
    assert L.fs_passages(0, u32, u32, u32, f64, f64, 1, 0, 0, None, 0, C.byref(n)) == abi.FS_E_INVALID
    assert L.fs_passages(0, u32, u32, u32, f64, f64, 1 << 32, 6, 0, None, 0,
                         C.byref(n)) == abi.FS_E_UNSUPPORTED
    assert L.fs_passages(0, None, None, None, None, None, 0, 6, 0, None, 0, C.byref(n)) == abi.FS_OK
    assert n.value == 0
    assert L.fs_passages_rows(None, None, 0, 6, 0, None, 0, C.byref(n)) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

@pytest.mark.parametrize("case,src,m,g", mpg.CASES)
def test_golden_passages_are_the_oracle_output(case, src, m, g):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    with open(os.path.join(gold, mpg.golden_name(case, m, g)), newline="", encoding="utf-8") as fh:
        want = fh.read()
    assert pr.passages_csv(text, m, g) == want
    assert want.count("\r\n") > 1                       # every case has passages
