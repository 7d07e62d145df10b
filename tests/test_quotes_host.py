"""`ao3.py quotes` without a GPU: the oracle's known answers, the parser, the C ABI's
declarations and the committed expected CSVs."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import passages_restated as pr
from tests import quotes_restated as qr
from tests.golden import make_quotes_golden as mqg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _rec(work, fan, orig, comb=0.0):
    return (work, fan, orig, 0.0, comb)


def _diag(work, fan0, orig0, n, comb=0.0):
    return [_rec(work, fan0 + k, orig0 + k, comb) for k in range(n)]


def _word(n_words=0, n_exact=0, n_works=0, n_passages=0, n_passage_works=0, region=qr.NONE):
    return dict(n_words=n_words, n_exact=n_exact, n_works=n_works, n_passages=n_passages,
                n_passage_works=n_passage_works, region=region)


# ---- oracle known answers -------------------------------------------------------------

def test_two_works_quoting_overlapping_spans():
    recs = _diag(0, 5, 10, 8) + _diag(1, 0, 14, 8, comb=0.07)
    words, regions = qr.quotes(recs, 2, 24)
    assert regions == [dict(first=10, last=21, n_passages=2, n_works=2, n_words=16, n_exact=8,
                            peak=2, peak_first=14, peak_last=17)]
    assert words[9] == _word() and words[22] == _word()
    assert words[10] == _word(1, 1, 1, 1, 1, 0)
    assert words[14] == words[17] == _word(2, 1, 2, 2, 2, 0)
    assert words[18] == _word(1, 0, 1, 1, 1, 0)


def test_one_work_quoting_a_line_twice_has_depth_one():
    recs = _diag(0, 0, 10, 6) + _diag(0, 20, 10, 6)
    words, regions = qr.quotes(recs, 1, 16)
    assert all(words[o] == _word(2, 2, 1, 2, 1, 0) for o in range(10, 16))
    assert regions == [dict(first=10, last=15, n_passages=2, n_works=1, n_words=12, n_exact=12,
                            peak=1, peak_first=10, peak_last=15)]
    # ... and two works quoting it once each have depth two
    words, regions = qr.quotes(_diag(0, 0, 10, 6) + _diag(1, 20, 10, 6), 2, 16)
    assert words[10] == _word(2, 2, 2, 2, 2, 0) and regions[0]["peak"] == 2


def test_a_stray_record_counts_in_n_words_but_in_no_region():
    recs = _diag(0, 0, 0, 6) + [_rec(0, 9, 30, NAN), _rec(1, 4, 30, -0.0), _rec(1, 5, 2, 0.3)]
    words, regions = qr.quotes(recs, 2, 31)
    assert words[30] == _word(2, 1, 2, 0, 0, qr.NONE)
    assert words[2] == _word(2, 1, 2, 1, 1, 0)
    assert regions == [dict(first=0, last=5, n_passages=1, n_works=1, n_words=7, n_exact=6,
                            peak=1, peak_first=0, peak_last=5)]


def test_min_works_two_splits_a_region():
    recs = _diag(0, 0, 0, 20) + _diag(1, 0, 2, 6) + _diag(2, 0, 12, 6) + _diag(3, 0, 30, 6)
    words, regions = qr.quotes(recs, 4, 36, min_works=1)
    assert regions == [
        dict(first=0, last=19, n_passages=3, n_works=3, n_words=32, n_exact=32, peak=2,
             peak_first=2, peak_last=7),
        dict(first=30, last=35, n_passages=1, n_works=1, n_words=6, n_exact=6, peak=1,
             peak_first=30, peak_last=35)]
    words, regions = qr.quotes(recs, 4, 36, min_works=2)
    # work 0's passage intersects both regions, work 3's none
    assert regions == [
        dict(first=2, last=7, n_passages=2, n_works=2, n_words=12, n_exact=12, peak=2,
             peak_first=2, peak_last=7),
        dict(first=12, last=17, n_passages=2, n_works=2, n_words=12, n_exact=12, peak=2,
             peak_first=12, peak_last=17)]
    assert [words[o]["region"] for o in (1, 2, 7, 8, 11, 12, 17, 18, 30)] == \
        [qr.NONE, 0, 0, qr.NONE, qr.NONE, 1, 1, qr.NONE, qr.NONE]
    assert words[30] == _word(1, 1, 1, 1, 1, qr.NONE)
    assert qr.quotes(recs, 4, 36, min_works=3) == (
        [dict(w, region=qr.NONE) for w in words], [])


def test_a_bridged_word_is_covered():
    recs = [_rec(0, f, f) for f in (0, 1, 2, 4, 5, 6)]
    assert qr.quotes(recs, 1, 7)[1] == []                      # no passage without the gap
    words, regions = qr.quotes(recs, 1, 7, max_gap=1)
    assert words[3] == _word(0, 0, 0, 1, 1, 0)
    assert regions == [dict(first=0, last=6, n_passages=1, n_works=1, n_words=6, n_exact=6,
                            peak=1, peak_first=0, peak_last=6)]


def test_the_peak_run_is_the_first_one():
    # depth 1 2 2 1 2 2 2 1 over words 0..7: the peak's run is the first, not the longest
    recs = _diag(0, 0, 0, 8) + _diag(1, 0, 1, 2) + _diag(2, 0, 4, 3)
    _, regions = qr.quotes(recs, 3, 8, min_words=2)
    assert (regions[0]["peak"], regions[0]["peak_first"], regions[0]["peak_last"]) == (2, 1, 2)


def test_refusals_and_no_records():
    ok = _diag(0, 0, 0, 3)
    for kw in (dict(min_words=0), dict(min_works=0), dict(n_works=0), dict(n_script=2)):
        args = dict(n_works=1, n_script=3, min_words=1, min_works=1)
        args.update(kw)
        with pytest.raises(ValueError):
            qr.quotes(ok, **args)
    with pytest.raises(ValueError):
        qr.quotes([_rec(0, 1, 0), _rec(0, 0, 1)], 1, 3)
    assert qr.quotes([], 2, 2) == ([_word(), _word()], [])


def _row(name, fan, orig, scene="1", char="ANNA", comb="0.0", word=None):
    return [name, fan, "f%d" % fan, 1, orig, word or "W%d" % orig, 2, char, scene, "0.0", 7, comb]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_two_files():
    rows = ([_row("b.txt", f, f + 10, scene="3", char="BOB") for f in (0, 1, 2, 4, 5, 6)] +
            [_row("a.txt", f, f + 8, scene="2" if f < 2 else "3", char="BOB") for f in range(6)] +
            [_row("a.txt", 50, 40, scene="9", char="ZED", comb="0.25")])
    quotes, words = qr.quotes_csv(_match_csv(rows), 6, 1)
    assert quotes.split("\r\n")[1:] == [
        "8,16,9,BOB,2,2,2,12,12,2,10,13,W8 W9 W10 W11 W12 W13 W14 W15 W16", ""]
    assert words.split("\r\n")[1:] == [
        "8,W8,1,1,1,1,1,1", "9,W9,1,1,1,1,1,1", "10,W10,2,2,2,2,2,1", "11,W11,2,2,2,2,2,1",
        "12,W12,2,2,2,2,2,1", "13,W13,1,1,1,2,2,1", "14,W14,1,1,1,1,1,1", "15,W15,1,1,1,1,1,1",
        "16,W16,1,1,1,1,1,1", "40,W40,1,0,1,0,0,", ""]
    assert qr.quotes_csv(_match_csv(rows, header=False), 6, 1) == (quotes, words)
    # at two works the bridged word, which a.txt names, is inside: nothing unknown is left
    quotes2, _ = qr.quotes_csv(_match_csv(rows), 6, 1, 2)
    assert quotes2.split("\r\n")[1:] == ["10,13,4,BOB,3,2,2,7,7,2,10,13,W10 W11 W12 W13", ""]


def test_a_bridged_word_without_a_record_is_written_as_unknown():
    rows = [_row("b.txt", f, f + 10) for f in (0, 1, 2, 4, 5, 6)]
    quotes, words = qr.quotes_csv(_match_csv(rows), 6, 1)
    assert quotes.split("\r\n")[1] == "10,16,7,ANNA,1,1,1,6,6,1,10,16,W10 W11 W12 [?] W14 W15 W16"
    assert words.split("\r\n")[4] == "13,[?],0,0,0,1,1,1"


def test_a_script_word_with_two_labels_is_an_error():
    from fandom_search_amd import quotes
    for other in (dict(scene="4"), dict(char="BOB"), dict(word="other")):
        rows = [_row("a.txt", 0, 5), _row("a.txt", 1, 6), _row("b.txt", 0, 5, **other)]
        with pytest.raises(ValueError):
            qr.quotes_csv(_match_csv(rows))
        with pytest.raises(ValueError, match="script word 5 "):
            quotes.word_labels([[str(c) for c in r] for r in rows])


def test_empty_input():
    quotes, words = qr.quotes_csv("")
    assert quotes == ",".join(qr.REGION_FIELDS) + "\r\n"
    assert words == ",".join(qr.WORD_FIELDS) + "\r\n"


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import quotes
    args = cli.build_parser().parse_args(["quotes", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_quotes"
    assert (args.output, args.min_words, args.max_gap, args.min_works, args.device) == \
        (None, 6, 0, 1, 0)
    assert quotes.output_names(args.matches) == ("runs/match-6gram-20240101-quotes.csv",
                                                 "runs/match-6gram-20240101-quotes-words.csv")
    assert quotes.output_names("batch", None)[0] == "batch-quotes.csv"
    assert quotes.output_names("m.csv", "out/x")[1] == "out/x-quotes-words.csv"
    args = cli.build_parser().parse_args(["quotes", "m.csv", "-o", "p", "--min-words", "3",
                                          "--max-gap", "2", "--min-works", "4", "--device", "1"])
    assert (args.output, args.min_words, args.max_gap, args.min_works, args.device) == \
        ("p", 3, 2, 4, 1)
    assert quotes.REGION_FIELDS == qr.REGION_FIELDS
    assert quotes.WORD_FIELDS == qr.WORD_FIELDS
    assert quotes.UNKNOWN_WORD == qr.UNKNOWN_WORD == "[?]"


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--max-gap", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["quotes", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py quotes: error: ")


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_quotes_entry_points():
    for name in ("fs_quotes", "fs_quotes_rows"):
        assert name in _declared_functions()
        assert name in _lib.SYMBOLS
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    assert hasattr(lib, "fs_quotes") and hasattr(lib, "fs_quotes_rows")


@pytest.mark.parametrize("struct,dtype,size,keys",
                         [("fs_quote_word", "QUOTE_WORD_DTYPE", 24, qr.WORD_KEYS),
                          ("fs_quote_region", "QUOTE_REGION_DTYPE", 40,
                           qr.REGION_KEYS + ["reserved"])])
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


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    d = np.zeros(1, dtype=np.float64)
    words = np.ones(4, dtype=abi.QUOTE_WORD_DTYPE)
    u32, f64 = abi.ptr(z, C.c_uint32), abi.ptr(d, C.c_double)
    w = words.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, min_words=6, min_works=1, words=w, cap=0, n_regions=C.byref(n)):
        return L.fs_quotes(0, u32, u32, u32, f64, n_rows, 2, n_script, min_words, 0, min_works,
                           words, None, cap, n_regions)
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_works=0) == abi.FS_E_INVALID
    assert b"at least 1" in L.fs_last_error()
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(words=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                     # a capacity without a buffer
    assert call(n_regions=None) == abi.FS_E_INVALID
    # no records: empty words without device work
    assert call(n_rows=0) == abi.FS_OK and n.value == 0
    assert (words["region"] == qr.NONE).all()
    assert not any(words[name].any() for name in qr.WORD_KEYS[:-1])
    assert L.fs_quotes_rows(None, None, 0, 0, 6, 0, 1, None, None, 0,
                            C.byref(n)) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_cases_are_those_of_the_issue():
    assert len(mqg.CASES) == 14 and {c[4] for c in mqg.CASES} == {1, 2}
    assert {c[0] for c in mqg.CASES} == set(mqg.NAMES)


@pytest.mark.parametrize("case,src,m,g,k", mqg.CASES)
def test_golden_files_are_the_oracle_output(case, src, m, g, k):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    got = qr.quotes_csv(text, m, g, k)
    for name, part in zip(mqg.golden_names(case, m, g, k), got):
        with open(os.path.join(gold, name), newline="", encoding="utf-8") as fh:
            want = fh.read()
        assert part == want, name
        assert want.count("\r\n") > 1                   # every case has regions and words
