"""`ao3.py readings` without a GPU: the oracle's known answers (tests/readings_restated.py), the
parser, the C ABI's declarations and the committed expected CSVs."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import passages_restated as pr
from tests import readings_restated as rr
from tests.golden import make_readings_golden as mrg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def quote(work, fan, orig, spells, skip=()):
    """Records (work, fan_ix, orig_ix, spell) of one quotation that starts at fan word `fan`
    and script word `orig`; positions in `skip` have no record."""
    out, k = [], 0
    for j in range(len(spells) + len(skip)):
        if j in skip:
            continue
        out.append((work, fan + j, orig + j, spells[k]))
        k += 1
    return out


def brief(found):
    return [(r["orig_first"], r["orig_last"], r["n_words"], r["n_passages"], r["n_works"],
             r["span"], r["rank"], r["first"]) for r in found]


# ---- oracle known answers -------------------------------------------------------------

LINE = [1, 2, 3, 4, 5, 6]


def test_two_works_with_the_same_line():
    recs = quote(0, 10, 50, LINE) + quote(1, 0, 50, LINE)
    found, spans, n = rr.readings(recs, 2, 60, 9)
    assert n == 2 and brief(found) == [(50, 55, 6, 2, 2, 0, 1, 0)]
    assert spans == [dict(orig_first=50, orig_last=55, n_passages=2, n_works=2, n_readings=1,
                          first_reading=0)]
    assert found[0]["reserved"] == 0 and list(found[0]) and set(found[0]) == set(rr.READING_KEYS)
    assert list(spans[0]) == rr.SPAN_KEYS


def test_one_word_changed_and_one_work_repeating_a_line():
    recs = (quote(0, 10, 50, LINE) + quote(0, 30, 50, LINE) + quote(0, 50, 50, LINE)
            + quote(1, 0, 50, LINE[:5] + [7]) + quote(2, 0, 50, LINE[:5] + [7]))
    found, spans, n = rr.readings(recs, 3, 60, 9)
    # two works beat three passages of one work
    assert n == 5 and brief(found) == [(50, 55, 6, 2, 2, 0, 1, 18), (50, 55, 6, 3, 1, 0, 2, 0)]
    assert spans[0]["n_passages"] == 5 and spans[0]["n_works"] == 3 and spans[0]["n_readings"] == 2


def test_the_same_fan_words_at_two_spans_and_a_prefix():
    recs = (quote(0, 0, 50, LINE) + quote(0, 20, 20, LINE) + quote(1, 0, 50, LINE + [7])
            + quote(2, 0, 20, LINE))
    found, spans, _ = rr.readings(recs, 3, 60, 9)
    assert brief(found) == [(20, 25, 6, 2, 2, 0, 1, 6), (50, 55, 6, 1, 1, 1, 1, 0),
                            (50, 56, 7, 1, 1, 2, 1, 12)]
    assert [(s["orig_first"], s["orig_last"], s["first_reading"]) for s in spans] == \
        [(20, 25, 0), (50, 55, 1), (50, 56, 2)]


def test_max_gap_bridging_different_words_over_one_span():
    recs = (quote(0, 0, 50, LINE, skip=(2,)) + quote(1, 0, 50, LINE, skip=(3,))
            + quote(2, 0, 50, LINE, skip=(2,)))
    assert rr.readings(recs, 3, 60, 9, 6, 0)[2] == 0
    found, spans, n = rr.readings(recs, 3, 60, 9, 6, 1)
    assert n == 3 and brief(found) == [(50, 56, 6, 2, 2, 0, 1, 0), (50, 56, 6, 1, 1, 0, 2, 6)]
    assert len(spans) == 1 and spans[0]["n_works"] == 3


def test_ties_and_a_span_whose_readings_share_works():
    recs = (quote(0, 0, 50, LINE) + quote(0, 20, 50, LINE[:5] + [8])
            + quote(1, 0, 50, LINE[:5] + [7]) + quote(1, 20, 50, LINE[:5] + [8])
            + quote(1, 40, 50, LINE))
    found, spans, _ = rr.readings(recs, 2, 60, 9)
    # works 2, 2, 1; equal works and passages: the earlier first record
    assert brief(found) == [(50, 55, 6, 2, 2, 0, 1, 0), (50, 55, 6, 2, 2, 0, 2, 6),
                            (50, 55, 6, 1, 1, 0, 3, 12)]
    assert spans[0]["n_works"] == 2 < sum(r["n_works"] for r in found)


def test_refusals_and_no_records():
    good = quote(0, 0, 0, LINE)
    for bad in ((1, 9, 9, 0), (0, 9, 20, 0), (0, 9, 9, 9)):
        with pytest.raises(ValueError):
            rr.readings(good + [bad], 1, 20, 9)
    with pytest.raises(ValueError):
        rr.readings(good[::-1], 1, 20, 9)
    with pytest.raises(ValueError):
        rr.readings(good, 1, 20, 9, min_words=0)
    with pytest.raises(NotImplementedError):
        rr.readings([], 1, (1 << 19) + 1, 1)
    assert rr.readings([], 0, 0, 0) == ([], [], 0)
    assert rr.readings(good, 1, 20, 9, min_words=7) == ([], [], 0)


def _row(name, fan, fan_word, orig, word, char="HAN", scene="4"):
    return [name, fan, fan_word, 1, orig, word, 2, char, scene, "0.0", 7, "0.0"]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


SCRIPT = "never tell me the odds".split()


def _quote_rows(name, fan, words):
    return [_row(name, fan + k, w, 7 + k, SCRIPT[k]) for k, w in enumerate(words)]


ROWS = (_quote_rows("b.txt", 5, SCRIPT) + _quote_rows("a.txt", 0, ["Never"] + SCRIPT[1:])
        + _quote_rows("c.txt", 0, SCRIPT) + _quote_rows("b.txt", 40, SCRIPT[:4] + ["odds!"]))


def test_the_two_files():
    found, spans = rr.readings_csv(_match_csv(ROWS), min_words=5)
    assert found.split("\r\n")[1:] == [
        "7,11,5,HAN,4,1,2,2,0,1,b.txt,never tell me the odds,never tell me the odds",
        "7,11,5,HAN,4,2,1,1,1,0,b.txt,never tell me the odds!,never tell me the odds",
        "7,11,5,HAN,4,3,1,1,1,0,a.txt,Never tell me the odds,never tell me the odds", ""]
    assert spans.split("\r\n")[1:] == [
        "7,11,5,HAN,4,4,3,3,2,never tell me the odds,2,never tell me the odds", ""]
    assert rr.readings_csv(_match_csv(ROWS, header=False), min_words=5) == (found, spans)
    assert rr.readings_csv(_match_csv(ROWS)) == tuple(
        ",".join(f) + "\r\n" for f in (rr.READING_FIELDS, rr.SPAN_FIELDS))


def test_fold_case_merges_and_shows_the_first_passage():
    found, spans = rr.readings_csv(_match_csv(ROWS), min_words=5, fold_case=True)
    assert found.split("\r\n")[1:3] == [
        "7,11,5,HAN,4,1,3,3,0,1,b.txt,never tell me the odds,never tell me the odds",
        "7,11,5,HAN,4,2,1,1,1,0,b.txt,never tell me the odds!,never tell me the odds"]
    assert spans.split("\r\n")[1] == \
        "7,11,5,HAN,4,4,3,2,3,never tell me the odds,3,never tell me the odds"


def test_top_and_min_works_leave_the_spans_file_alone():
    base = rr.readings_csv(_match_csv(ROWS), min_words=5, top=0)
    for cut in (rr.readings_csv(_match_csv(ROWS), min_words=5, top=1),
                rr.readings_csv(_match_csv(ROWS), min_words=5, min_works=2)):
        assert cut[1] == base[1]
        assert cut[0].split("\r\n")[1:] == base[0].split("\r\n")[1:2] + [""]
    # a rank is the reading's place among all readings of the span
    both = rr.readings_csv(_match_csv(ROWS + _quote_rows("d.txt", 0, ["Never"] + SCRIPT[1:])),
                           min_words=5, top=2, min_works=2)
    assert [r.split(",")[5:8] for r in both[0].split("\r\n")[1:3]] == [["1", "2", "2"], ["2", "2", "2"]]


def test_a_bridged_word_without_a_record_is_unknown_in_the_span_text():
    rows = [r for r in ROWS[:5] if r[4] != 9] + [r for r in ROWS[5:10] if r[4] != 9]
    found, spans = rr.readings_csv(_match_csv(rows), min_words=4, max_gap=1)
    assert found.split("\r\n")[1].endswith(",never tell the odds,never tell the odds")
    assert spans.split("\r\n")[1].endswith(",never tell [?] the odds")


def test_a_script_word_with_two_labels_is_an_error():
    rows = ROWS + [_row("c.txt", 90, "x", 8, "tell", scene="9")]
    with pytest.raises(ValueError, match="script word 8 has two scenes"):
        rr.readings_csv(_match_csv(rows))


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import readings
    args = cli.build_parser().parse_args(["readings", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_readings"
    assert (args.output, args.min_words, args.max_gap, args.top, args.min_works, args.fold_case,
            args.device, args.reader) == (None, 6, 0, 10, 1, False, 0, None)
    assert readings.output_names(args.matches) == (
        "runs/match-6gram-20240101-readings.csv", "runs/match-6gram-20240101-readings-spans.csv")
    assert readings.output_names("batch", None)[0] == "batch-readings.csv"
    assert readings.output_names("m.csv", "out/x")[1] == "out/x-readings-spans.csv"
    args = cli.build_parser().parse_args(
        ["readings", "m.csv", "-o", "p", "--min-words", "3", "--max-gap", "2", "--top", "0",
         "--min-works", "4", "--fold-case", "--device", "1", "--reader", "python"])
    assert (args.output, args.min_words, args.max_gap, args.top, args.min_works, args.fold_case,
            args.device, args.reader) == ("p", 3, 2, 0, 4, True, 1, "python")
    assert readings.READING_FIELDS == rr.READING_FIELDS and readings.SPAN_FIELDS == rr.SPAN_FIELDS


@pytest.mark.parametrize("bad", [["--top", "-1"], ["--min-works", "0"], ["--min-words", "0"],
                                 ["--max-gap", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["readings", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py readings: error: ")


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_readings", "fs_readings_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "fs_readings_rows" not in declared and "no\n * _rows twin" in text


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_reading", "READING_DTYPE", rr.READING_KEYS, 40),
    ("fs_reading_span", "READING_SPAN_DTYPE", rr.SPAN_KEYS, 24)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for kind, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body):
        for n in names.split(","):
            fields.append((n.strip(), at))
            at += 8 if kind == "uint64_t" else 4
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert list(dt.names) == keys
    assert "#define FS_READINGS_MAX_BYTES (1u << 30)" in text and abi.FS_READINGS_MAX_BYTES == 1 << 30
    assert "#define FS_READINGS_SLOT_BYTES %du" % abi.FS_READINGS_SLOT_BYTES in text


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    got = [C.c_uint64(7) for _ in range(3)]
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    found = np.ones(4, dtype=abi.READING_DTYPE)
    f = found.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, min_words=1, readings=f, cap=4, spans=None, cap_spans=0,
             outs=None):
        outs = [C.byref(g) for g in got] if outs is None else outs
        return L.fs_readings(0, u32, u32, u32, u32, n_rows, 2, n_script, 2, min_words, 0, readings,
                             cap, spans, cap_spans, *outs)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(readings=None) == abi.FS_E_INVALID            # a capacity without a buffer
    assert call(cap_spans=1) == abi.FS_E_INVALID
    for k in range(3):
        outs = [C.byref(g) for g in got]
        outs[k] = None
        assert call(outs=outs) == abi.FS_E_INVALID
    # no records: zeros without device work
    assert call(n_rows=0) == abi.FS_OK and [g.value for g in got] == [0, 0, 0]
    assert (found["n_words"] == 1).all()
    assert L.fs_readings_times(None) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_golden_generator_reproduces_its_committed_files():
    made = mrg.build()
    assert set(made) == {mrg.INPUT} | {n for c in mrg.CASES for n in mrg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


def test_the_golden_input_holds_what_its_generator_says():
    rows = pr.read_rows(mrg.input_csv())
    assert 100 <= len(rows) <= 200
    names = [r[0] for r in rows]
    blocks = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
    assert len(blocks) > len(set(blocks))                      # a work comes back
    fans = {r[2] for r in rows}
    assert any("," in f for f in fans) and any('"' in f for f in fans)
    assert any(not f.isascii() for f in fans)
    found = mrg.build()[mrg.golden_names("default")[0]].split("\r\n")
    assert "100,107,8,HAN,4,1,4,3,0,1,a.txt,i have a very bad feeling about this," \
           "i have a very bad feeling about this" in found
    assert any(r.startswith("100,105,6,") for r in found)      # a prefix is a span of its own
    gap = mrg.build()[mrg.golden_names("gap1_top2_min2")[1]].split("\r\n")
    # five quotations of four works: two bridgings, one of them also with "Never", and the whole
    assert any(r.startswith("120,124,5,HAN,9,5,4,4,4,") for r in gap)
