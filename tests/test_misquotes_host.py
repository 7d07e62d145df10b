"""`ao3.py misquotes` without a GPU: the restated contract (tests/misquotes_restated.py) on
examples worked by hand, the parser, the refusals, the C ABI's declarations and the committed
expected CSVs."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, misquotes
from tests import misquotes_restated as mr
from tests.golden import make_misquotes_golden as mmg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def records_of(quotes, n=6):
    """Records (work, fan_ix, orig_ix, spell) of quotations (work, first script word, {offset:
    spelling}) of `n` words; script word o is spelt o unless the dict says otherwise."""
    recs, at = [], {}
    for w, o0, changed in sorted(quotes, key=lambda q: q[0]):
        f = at.get(w, 0)
        recs += [(w, f + k, o0 + k, changed.get(k, o0 + k)) for k in range(n)]
        at[w] = f + n + 10
    return recs


def run(quotes, n_works, n_script=40, n=6, **kw):
    same = list(range(n_script))
    return mr.misquotes(records_of(quotes, n), same, n_works, 1000, **kw)


# ---- the restatement on examples worked by hand --------------------------------------------

def test_telling_bound_both_sides():
    # readers 8: four works are telling at 50, five are not
    assert mr.is_telling(4, 8, 50) and not mr.is_telling(5, 8, 50)
    # readers 3, works 2: 200 > 198 at 66, 200 <= 201 at 67
    assert not mr.is_telling(2, 3, 66) and mr.is_telling(2, 3, 67)
    assert mr.is_telling(3, 3, 100) and not mr.is_telling(3, 3, 99)
    assert mr.is_telling(1, 100, 1) and not mr.is_telling(1, 99, 1)
    # through the whole restatement: 8 readers of word 12, works 0..3 and works 0..4
    for k, want in ((4, 1), (5, 0)):
        quotes = [(w, 10, {2: 900} if w < k else {}) for w in range(8)]
        _, found, pairs = run(quotes, 8)
        assert [(m["works"], m["readers"], m["telling"]) for m in found] == [(k, 8, want)]
        assert len(pairs) == (6 if want else 0)
    quotes = [(0, 10, {2: 900}), (1, 10, {2: 900}), (2, 10, {})]
    assert run(quotes, 3, max_share=66)[1][0]["telling"] == 0
    assert run(quotes, 3, max_share=67)[1][0]["telling"] == 1


def test_weight_rule():
    assert mr.weight_of(5, 5) == 1 and mr.weight_of(3, 5) == 1          # readers // works = 1
    assert mr.weight_of(2, 5) == 2 and mr.weight_of(2, 4) == 2          # 2
    assert mr.weight_of(2, 7) == 2                                      # 3
    assert mr.weight_of(2, 8) == 3
    assert mr.weight_of(1, 2 ** 31) == 32 and mr.weight_of(1, 2 ** 31 - 1) == 31
    assert all(mr.weight_of(k, r, "flat") == 1 for k, r in ((1, 1), (2, 9), (1, 2 ** 31)))
    with pytest.raises(ValueError):
        mr.weight_of(1, 2, "idf")
    # a misquote that is not telling weighs nothing
    quotes = [(w, 10, {2: 900} if w < 2 else {}) for w in range(3)]
    assert [m["weight"] for m in run(quotes, 3)[1]] == [0]
    assert [m["weight"] for m in run(quotes, 3, max_share=100)[1]] == [1]


def test_agreement_formula():
    assert mr.agreement(1, 1, 1) == 100
    assert mr.agreement(2, 3, 2) == 66
    assert mr.agreement(1, 3, 1) == 33
    assert mr.agreement(1, 4, 3) == 16


def test_a_family_and_a_bystander():
    # works 0 and 1 copy two misquotes, 2 shares one of them, 3 and 4 quote verbatim; work 5
    # has the same wrong word in a run that is too short
    quotes = [(0, 10, {1: 901, 4: 902}), (1, 10, {1: 901, 4: 902}), (2, 10, {4: 902, 5: 903}),
              (3, 10, {}), (4, 10, {})]
    recs = records_of(quotes) + [(5, k, 10 + k, 901 if k == 1 else 10 + k) for k in range(5)]
    works, found, pairs = mr.misquotes(recs, list(range(40)), 6, 1000)
    assert [(m["orig_ix"], m["spell"], m["records"], m["works"], m["readers"], m["telling"],
             m["weight"], m["first_work"]) for m in found] == \
        [(11, 901, 2, 2, 5, 1, 2, 0), (14, 902, 3, 3, 5, 0, 0, 0)]
    assert pairs == [dict(a=0, b=1, shared=1, score=2, a_on_common=1, b_on_common=1, strongest=0,
                          strongest_weight=2)]
    assert [w["passage_records"] for w in works] == [6, 6, 6, 6, 6, 0]
    assert [w["departures"] for w in works] == [2, 2, 2, 0, 0, 0]
    assert [w["misquotes"] for w in works] == [2, 2, 1, 0, 0, 0]
    assert [w["singular"] for w in works] == [0, 0, 1, 0, 0, 0]
    assert [w["closest"] for w in works] == [1, 0, NONE, NONE, NONE, NONE]
    # five words are a passage under --min-words 5: work 5 reads and departs
    works, found, pairs = mr.misquotes(recs, list(range(40)), 6, 1000, min_words=5)
    assert found[0]["works"] == 3 and found[0]["readers"] == 6
    assert [m["telling"] for m in found] == [1, 1] and len(pairs) == 5


def test_on_common_counts_only_ground_both_quote():
    # work 0 departs at 11 and at 31; work 1 shares the first and never quotes the second line
    quotes = [(0, 10, {1: 901}), (0, 30, {1: 905}), (1, 10, {1: 901}), (2, 30, {1: 905}),
              (3, 10, {}), (3, 30, {}), (4, 10, {}), (4, 30, {})]
    _, found, pairs = run(quotes, 5)
    by = {(p["a"], p["b"]): p for p in pairs}
    assert (by[0, 1]["a_on_common"], by[0, 1]["b_on_common"], by[0, 1]["shared"]) == (1, 1, 1)
    assert (by[0, 2]["a_on_common"], by[0, 2]["b_on_common"]) == (1, 1)
    assert set(by) == {(0, 1), (0, 2)}


def test_strongest_ties_go_to_the_smallest_number_and_closest_to_the_earlier_work():
    quotes = [(0, 10, {0: 900, 3: 901}), (1, 10, {0: 900, 3: 901}), (2, 10, {0: 900, 3: 901})] + \
        [(w, 10, {}) for w in range(3, 9)]
    works, found, pairs = run(quotes, 9)
    assert [m["weight"] for m in found] == [2, 2]
    assert all(p["strongest"] == 0 and p["score"] == 4 for p in pairs) and len(pairs) == 3
    assert [works[w]["closest"] for w in range(3)] == [1, 0, 0]
    assert run(quotes, 9, min_score=5)[2] == [] and run(quotes, 9, min_shared=3)[2] == []


def test_a_bridged_word_has_no_reader_in_the_bridging_work():
    recs = records_of([(0, 10, {2: 900}), (1, 10, {2: 900}), (2, 10, {})])
    recs += [(3, k, 10 + k, 10 + k) for k in range(6) if k != 2]
    _, found, _ = mr.misquotes(recs, list(range(40)), 4, 1000, min_words=5, max_gap=1,
                               max_share=100)
    assert [(m["works"], m["readers"]) for m in found] == [(2, 3)]


def test_refusals_of_the_restatement():
    recs = records_of([(0, 10, {}), (1, 10, {})])
    same = list(range(40))
    for kw in (dict(min_works=1), dict(max_share=0), dict(max_share=101), dict(min_shared=0),
               dict(min_score=0), dict(min_words=0), dict(max_gap=-1), dict(weight="idf")):
        with pytest.raises(ValueError):
            mr.misquotes(recs, same, 2, 1000, **kw)
    with pytest.raises(ValueError):
        mr.misquotes(recs, same, 1, 1000)
    with pytest.raises(ValueError):
        mr.misquotes(recs, same[:15], 2, 1000)
    with pytest.raises(ValueError):
        mr.misquotes(recs, same, 2, 15)                 # a spell and a same[] above n_spell
    with pytest.raises(ValueError):
        mr.misquotes(recs[::-1], same, 2, 1000)
    with pytest.raises(NotImplementedError):
        mr.misquotes(recs, [NONE] * ((1 << 19) + 1), 2, 1000)


# ---- the parser ----------------------------------------------------------------------------

def test_parser_defaults_and_options():
    args = cli.ao3_parser().parse_args(["misquotes", "runs/m.csv"])
    assert (args.min_words, args.max_gap, args.min_works, args.max_share, args.weight,
            args.min_shared, args.min_score, args.keep_case, args.device, args.reader,
            args.output) == (6, 0, 2, 50, "rarity", 1, 1, False, 0, None, None)
    assert misquotes.output_names(args.matches, args.output) == (
        "runs/m-misquotes.csv", "runs/m-misquotes-pairs.csv", "runs/m-misquotes-works.csv")
    args = cli.ao3_parser().parse_args(
        ["misquotes", "m.csv", "-o", "out/x", "--min-words", "4", "--max-gap", "1", "--min-works",
         "3", "--max-share", "100", "--weight", "flat", "--min-shared", "2", "--min-score", "3",
         "--keep-case", "--device", "1", "--reader", "python"])
    assert (args.min_words, args.max_gap, args.min_works, args.max_share, args.weight,
            args.min_shared, args.min_score, args.keep_case, args.device, args.reader) == \
        (4, 1, 3, 100, "flat", 2, 3, True, 1, "python")
    assert misquotes.output_names(args.matches, args.output)[1] == "out/x-misquotes-pairs.csv"
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["misquotes", "m.csv", "--weight", "idf"])
    assert "misquotes" in cli.ao3_parser().format_help()
    assert misquotes.MISQUOTE_FIELDS == mr.MISQUOTE_FIELDS and misquotes.PAIR_FIELDS == \
        mr.PAIR_FIELDS and misquotes.WORK_FIELDS == mr.WORK_FIELDS


@pytest.mark.parametrize("bad,message", [
    (["--min-works", "1"], "--min-works must be at least 2"),
    (["--max-share", "0"], "--max-share must be from 1 to 100"),
    (["--max-share", "101"], "--max-share must be from 1 to 100"),
    (["--min-shared", "0"], "--min-shared and --min-score must be at least 1"),
    (["--min-score", "0"], "--min-shared and --min-score must be at least 1"),
    (["--min-words", "0"], "--min-words must be at least 1, --max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words must be at least 1, --max-gap at least 0")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["misquotes", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py misquotes: error: " + message


# ---- the C ABI -----------------------------------------------------------------------------

def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_misquotes", "fs_misquotes_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "fs_misquotes_rows" not in declared and "misquotes" in _lib.TIMED
    assert abi.MISQUOTES_MS_NAMES == ("passages", "cells", "number", "postings", "expand",
                                      "place", "detail", "total")
    assert re.search(r"#define FS_MISQUOTES_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_MISQUOTES_SLOT_BYTES 32u", text)
    assert re.search(r"#define FS_MISQUOTES_RECORD_SLOT_BYTES 40u", text)
    assert (abi.FS_MISQUOTES_MAX_BYTES, abi.FS_MISQUOTES_SLOT_BYTES,
            abi.FS_MISQUOTES_RECORD_SLOT_BYTES, abi.FS_MISQUOTES_RARITY, abi.FS_MISQUOTES_FLAT,
            abi.FS_MISQUOTES_MAX_ROWS) == (1 << 30, 32, 40, 0, 1, mr.MAX_ROWS)
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    body = open(os.path.join(src, "fs_misquotes.hip")).read()
    # the sets, scans and run heads are the shared ones; integer atomics only, no assembly
    assert '#include "fs_probe.h"' in body and '#include "fs_prims.h"' in body
    assert "fs_runs_find_cols(" in body and "fs_probe_insert(" in body and "scan_chunks<" in body
    assert "asm" not in body
    assert "fs_misquotes.hip" in open(os.path.join(src, "Makefile")).read()


@pytest.mark.parametrize("struct,dtype,keys", [
    ("fs_misquote", "MISQUOTE_DTYPE", mr.MISQUOTE_KEYS),
    ("fs_misquote_pair", "MISQUOTE_PAIR_DTYPE", mr.PAIR_KEYS),
    ("fs_misquote_work", "MISQUOTE_WORK_DTYPE", mr.WORK_KEYS)])
def test_dtypes_match_the_header(struct, dtype, keys):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for names in re.findall(r"\buint32_t\s+([^;]+);", body)
              for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == 32 == 4 * len(fields)
    assert list(dt.names) == fields == keys
    assert all(dt.fields[n] == (np.dtype(np.uint32), 4 * k) for k, n in enumerate(fields))


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    works = np.ones(2, dtype=abi.MISQUOTE_WORK_DTYPE)
    wp = works.ctypes.data_as(C.c_void_p)
    n_m, n_p = C.c_uint64(7), C.c_uint64(7)

    def call(n_rows=1, n_works=2, n_script=4, min_words=1, max_gap=0, min_works=2, max_share=50,
             weight=0, min_shared=1, min_score=1, works=wp, cap_m=0, cap_p=0, got_m=C.byref(n_m),
             got_p=C.byref(n_p), cols=u32):
        return L.fs_misquotes(0, cols, cols, cols, cols, cols, n_rows, n_works, n_script, 5,
                              min_words, max_gap, min_works, max_share, weight, min_shared,
                              min_score, works, None, cap_m, got_m, None, cap_p, got_p)
    assert call(n_rows=1 << 27) == abi.FS_E_UNSUPPORTED
    assert b"2^27" in L.fs_last_error()
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    for bad in (dict(min_words=0), dict(min_works=1), dict(min_works=0), dict(max_share=0),
                dict(max_share=101), dict(weight=2), dict(min_shared=0), dict(min_score=0),
                dict(works=None), dict(cap_m=1), dict(cap_p=1), dict(got_m=None),
                dict(got_p=None), dict(cols=None)):
        assert call(**bad) == abi.FS_E_INVALID, bad
    assert (works["departures"] == 1).all()                              # nothing written
    # no records: works without passages, without device work
    assert call(n_rows=0) == abi.FS_OK and (n_m.value, n_p.value) == (0, 0)
    assert works.tolist() == [(0, 0, 0, 0, 0, 0, NONE, 0)] * 2
    assert L.fs_misquotes_times(None) == abi.FS_E_INVALID
    ms = (C.c_double * 8)()
    assert L.fs_misquotes_times(ms) == abi.FS_OK and not any(ms)
    with pytest.raises(ValueError):
        misquotes.find_misquotes(z, z, z[:3], z, z, 2, 5)
    with pytest.raises(ValueError):
        misquotes.find_misquotes(z, z, z, z, z, 2, 5, weight="idf")


def test_same_spellings_of_the_host():
    labels = {3: ("Force", "A", "1"), 5: ("odds", "B", "2")}
    ids = {"force": 0, "the": 1}
    assert misquotes.same_spellings(labels, ids, 7, True).tolist() == \
        [NONE, NONE, NONE, 0, NONE, NONE, NONE]
    assert misquotes.same_spellings(labels, ids, 7, False).tolist() == [NONE] * 7


# ---- the committed expected files ----------------------------------------------------------

def test_goldens_are_what_the_generator_writes():
    for name, text in mmg.build().items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,options,kw", mmg.CASES)
def test_the_options_are_the_keywords(case, options, kw):
    args = cli.ao3_parser().parse_args(["misquotes", "m.csv"] + options)
    got = dict(min_words=args.min_words, max_gap=args.max_gap, min_works=args.min_works,
               max_share=args.max_share, weight=args.weight, min_shared=args.min_shared,
               min_score=args.min_score, keep_case=args.keep_case)
    assert {k: got[k] for k in kw} == kw


def test_what_the_golden_input_holds():
    import csv

    def rows(case, kind):
        name = mmg.golden_names(case)[mmg.KINDS.index(kind)]
        with open(os.path.join(GOLDEN, name), newline="", encoding="utf-8") as fh:
            return list(csv.DictReader(fh))
    mis = {r["FAN_WORK_WORD"]: r for r in rows("defaults", "misquotes")}
    assert mis["that"]["WORKS"] == "2" and mis["thé → 中"]["WORKS"] == "3"
    assert (mis["forse"]["TELLING"], mis["forse"]["SHARE_PERCENT"]) == ("0", "71")
    assert (mis["disturbin,"]["TELLING"], mis["disturbin,"]["SHARE_PERCENT"]) == ("1", "50")
    assert "May" not in mis and len({r["WEIGHT"] for r in mis.values()}) == 3
    # the tie of the strongest: two shared misquotes of one weight, the earlier script word wins
    ab = rows("defaults", "pairs")[0]
    assert (ab["SHARED"], ab["SCORE"], ab["STRONGEST_FAN_WORK_WORD"], ab["STRONGEST_WEIGHT"],
            ab["AGREEMENT_PERCENT"]) == ("2", "4", "that", "2", "66")
    keep = {r["FAN_WORK_WORD"]: r for r in rows("keepcase_flat_share100", "misquotes")}
    assert keep["May"]["WORKS"] == "2" and keep["forse"]["TELLING"] == "1"
    gap = {r["FAN_WORK_WORD"]: r for r in rows("gap1_words4_works3_shared2", "misquotes")}
    assert gap["that"]["WORKS"] == "3"                  # g.txt's run of five is a passage
    assert gap["baad"]["READERS"] == "6"                # f.txt bridges the word: no reader
    works = {r["FAN_WORK_FILENAME"]: r for r in rows("gap1_words4_works3_shared2", "works")}
    assert works["f.txt"]["PASSAGE_RECORDS"] == "23"
    assert len(rows("gap1_words4_works3_shared2", "pairs")) == 1
    # a file without records: three header rows
    from tests.passages_restated import MATCH_FIELDS
    assert mr.misquotes_csv(",".join(MATCH_FIELDS) + "\r\n") == tuple(
        ",".join(f) + "\r\n" for f in (mr.MISQUOTE_FIELDS, mr.PAIR_FIELDS, mr.WORK_FIELDS))
