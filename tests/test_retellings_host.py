"""`ao3.py retellings` without a GPU: the oracle's known answers worked by hand
(tests/retellings_restated.py), the parser, the C ABI's declarations, and the committed expected
CSVs under the product's table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, retellings
from fandom_search_amd.passages import read_matches
from tests import retellings_restated as rt
from tests.golden import make_retellings_golden as mrg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def work_of(spans, work=0, fan_gap=3):
    """Records (work, fan_ix, orig_ix) of passages (orig_first, words), one behind another in
    the work with `fan_gap` fan words between them."""
    out, fan = [], 0
    for orig, words in spans:
        out += [(work, fan + k, orig + k) for k in range(words)]
        fan += words + fan_gap
    return out


def column(rows, key):
    return [r[key] for r in rows]


# ---- oracle known answers, worked by hand ------------------------------------------------

def test_three_passages_ascending():
    works, found = rt.retellings(work_of([(10, 6), (20, 7), (30, 8)]), 1)
    assert column(found, "best") == [6, 13, 21] and column(found, "prev") == [NONE, 0, 1]
    assert column(found, "depth") == [1, 2, 3] == column(found, "chain_pos")
    assert column(found, "first") == [0, 6, 13]
    assert [(p["fan_first"], p["fan_last"], p["orig_first"], p["orig_last"]) for p in found] == \
        [(0, 5, 10, 15), (9, 15, 20, 26), (19, 26, 30, 37)]
    assert works == [dict(n_passages=3, passage_words=21, chain_passages=3, chain_words=21,
                          chain_first=0, chain_last=2, orig_first=10, orig_last=37,
                          chain_script_words=21, n_descents=0)]
    assert list(works[0]) == rt.WORK_KEYS and list(found[0]) == rt.PASSAGE_KEYS


def test_three_descending_with_equal_weights_the_chain_is_passage_0_alone():
    works, found = rt.retellings(work_of([(30, 6), (20, 6), (10, 6)]), 1)
    assert column(found, "best") == [6, 6, 6] and column(found, "prev") == [NONE] * 3
    assert column(found, "chain_pos") == [1, 0, 0]
    assert (works[0]["chain_first"], works[0]["chain_last"], works[0]["chain_passages"],
            works[0]["chain_words"], works[0]["n_descents"]) == (0, 0, 1, 6, 2)
    assert (works[0]["orig_first"], works[0]["orig_last"]) == (30, 35)


def test_touching_at_one_script_word_is_not_following_and_one_more_is():
    works, found = rt.retellings(work_of([(10, 6), (15, 6)]), 1)     # 15 == orig_last of passage 0
    assert column(found, "prev") == [NONE, NONE] and column(found, "chain_pos") == [1, 0]
    assert works[0]["chain_passages"] == 1 and works[0]["n_descents"] == 1
    works, found = rt.retellings(work_of([(10, 6), (16, 6)]), 1)
    assert column(found, "prev") == [NONE, 0] and column(found, "best") == [6, 12]
    assert works[0]["chain_passages"] == 2 and works[0]["n_descents"] == 0
    assert works[0]["chain_script_words"] == 12 and works[0]["orig_last"] == 21


def test_two_interleaved_sequences_of_equal_weight():
    # A = passages 0 and 2 (script words 100.., 110..), B = passages 1 and 3 (50.., 60..)
    works, found = rt.retellings(work_of([(100, 6), (50, 6), (110, 6), (60, 6)]), 1)
    assert column(found, "best") == [6, 6, 12, 12]
    # passage 2 may follow 0 and 1, both of best 6: the smaller j; passage 3 follows 1 only
    assert column(found, "prev") == [NONE, NONE, 0, 1]
    assert column(found, "depth") == [1, 1, 2, 2]
    # passages 2 and 3 end chains of 12 words: the smaller i
    assert (works[0]["chain_first"], works[0]["chain_last"]) == (0, 2)
    assert column(found, "chain_pos") == [1, 0, 2, 0]
    assert works[0]["n_descents"] == 2 and works[0]["chain_words"] == 12


def test_works_without_a_passage_and_passage_numbers_across_works():
    recs = work_of([(10, 6)], work=1) + work_of([(10, 5)], work=2) + \
        work_of([(40, 6), (50, 6)], work=4)
    works, found = rt.retellings(recs, 6)
    none = dict(n_passages=0, passage_words=0, chain_passages=0, chain_words=0, chain_first=NONE,
                chain_last=NONE, orig_first=0, orig_last=0, chain_script_words=0, n_descents=0)
    assert [w for w in range(6) if works[w] == none] == [0, 2, 3, 5]
    assert column(found, "work") == [1, 4, 4] and column(found, "prev") == [NONE, NONE, 1]
    assert (works[4]["chain_first"], works[4]["chain_last"]) == (1, 2)


def test_refusals_and_no_records():
    good = work_of([(0, 6)])
    with pytest.raises(ValueError):
        rt.retellings(good + [(1, 0, 0)], 1)
    with pytest.raises(ValueError):
        rt.retellings(good[::-1], 1)
    with pytest.raises(ValueError):
        rt.retellings(good, 1, min_words=0)
    assert rt.retellings([], 0) == ([], [])
    assert rt.retellings(good, 1, min_words=7)[1] == []


def _row(name, fan, fan_word, orig, word, char="HAN", scene="4"):
    return [name, fan, fan_word, 1, orig, word, 2, char, scene, "0.0", 7, "0.0"]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(rt.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_two_files_and_a_script_word_with_two_labels():
    odds, feel = "never tell me the odds".split(), "i have a bad feeling".split()
    rows = ([_row("b.txt", 5 + k, w, 7 + k, w) for k, w in enumerate(odds)]
            + [_row("a.txt", k, w, 30 + k, w, "LEIA", "9") for k, w in enumerate(feel)]
            + [_row("b.txt", 20 + k, w.upper(), 30 + k, w, "LEIA", "9") for k, w in enumerate(feel)])
    works, passages = rt.retellings_csv(_match_csv(rows), min_words=5)
    assert works.split("\r\n")[1:] == ["b.txt,2,10,2,10,100,0,7,34,28,10,5,24,2,4 > 9", ""]
    assert passages.split("\r\n")[1:] == [
        "b.txt,1,5,9,7,11,5,HAN,4,1,1,never tell me the odds,never tell me the odds",
        "b.txt,2,20,24,30,34,5,LEIA,9,1,2,I HAVE A BAD FEELING,i have a bad feeling", ""]
    assert rt.retellings_csv(_match_csv(rows, header=False), min_words=5) == (works, passages)
    one = rt.retellings_csv(_match_csv(rows), min_words=5, min_passages=1)
    assert [r.split(",")[0] for r in one[0].split("\r\n")[1:-1]] == ["b.txt", "a.txt"]
    assert rt.retellings_csv(_match_csv(rows)) == tuple(
        ",".join(f) + "\r\n" for f in (rt.WORK_FIELDS, rt.PASSAGE_FIELDS))
    with pytest.raises(ValueError, match="script word 8 has two scenes"):
        rt.retellings_csv(_match_csv(rows + [_row("c.txt", 90, "x", 8, "tell", scene="9")]))


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.build_parser().parse_args(["retellings", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_retellings"
    assert (args.output, args.min_words, args.max_gap, args.min_passages, args.min_share,
            args.device, args.reader) == (None, 6, 0, 2, 0, 0, None)
    assert retellings.output_names(args.matches) == (
        "runs/match-6gram-20240101-retellings.csv",
        "runs/match-6gram-20240101-retellings-passages.csv")
    assert retellings.output_names("batch", None)[0] == "batch-retellings.csv"
    assert retellings.output_names("m.csv", "out/x")[1] == "out/x-retellings-passages.csv"
    args = cli.build_parser().parse_args(
        ["retellings", "m.csv", "-o", "p", "--min-words", "3", "--max-gap", "2",
         "--min-passages", "4", "--min-share", "75", "--device", "1", "--reader", "python"])
    assert (args.output, args.min_words, args.max_gap, args.min_passages, args.min_share,
            args.device, args.reader) == ("p", 3, 2, 4, 75, 1, "python")
    assert retellings.WORK_FIELDS == rt.WORK_FIELDS
    assert retellings.PASSAGE_FIELDS == rt.PASSAGE_FIELDS
    assert "retellings" in cli.build_parser().format_help()


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-passages", "0"],
                                 ["--min-share", "-1"], ["--min-share", "101"],
                                 ["--max-gap", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["retellings", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py retellings: error: ")


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_retellings", "fs_retellings_rows", "fs_retellings_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert len(abi.RETELLINGS_MS_NAMES) == 6 and abi.RETELLINGS_MS_NAMES[-1] == "total"
    for name in ("FS_RETELLINGS_SMALL", "FS_RETELLINGS_LDS"):
        assert name in text
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_retelling", "RETELLING_DTYPE", rt.WORK_KEYS, 40),
    ("fs_retelling_passage", "RETELLING_PASSAGE_DTYPE", rt.PASSAGE_KEYS, 48)])
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


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    got = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    works = np.ones(2, dtype=abi.RETELLING_DTYPE)
    found = np.ones(4, dtype=abi.RETELLING_PASSAGE_DTYPE)
    wp, fp = works.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, min_words=1, out=wp, passages=fp, cap=4, n_out=C.byref(got), cols=u32):
        return L.fs_retellings(0, cols, cols, cols, n_rows, 2, min_words, 0, out, passages, cap,
                               n_out)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(passages=None) == abi.FS_E_INVALID            # a capacity without a buffer
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    # no records: summaries without a passage, no device work
    assert call(n_rows=0, cols=None, passages=None, cap=0) == abi.FS_OK and got.value == 0
    assert [tuple(w) for w in works.tolist()] == [(0, 0, 0, 0, NONE, NONE, 0, 0, 0, 0)] * 2
    assert (found["n_words"] == 1).all()
    assert L.fs_retellings_times(None) == abi.FS_E_INVALID
    for fn in (L.fs_retellings_rows,):
        assert fn(None, None, 0, 0, 1, 0, None, None, 0, C.byref(got)) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def as_arrays(works, found):
    w = np.array([tuple(r[k] for k in rt.WORK_KEYS) for r in works], dtype=abi.RETELLING_DTYPE)
    p = np.array([tuple(r[k] for k in rt.PASSAGE_KEYS) for r in found],
                 dtype=abi.RETELLING_PASSAGE_DTYPE)
    return w, p


def oracle_find(work, fan_ix, orig_ix, n_works, min_words=6, max_gap=0, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    return as_arrays(*rt.retellings(recs, n_works, min_words, max_gap))


def test_the_golden_generator_reproduces_its_committed_files():
    made = mrg.build()
    assert set(made) == {mrg.INPUT} | {n for c in mrg.CASES for n in mrg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,min_words,max_gap,min_passages,min_share", mrg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, min_words, max_gap,
                                                      min_passages, min_share):
    monkeypatch.setattr(retellings, "find_retellings", oracle_find)
    body = retellings.tables(read_matches(os.path.join(GOLDEN, mrg.INPUT)), min_words, max_gap,
                             min_passages, min_share)
    for name, head, part in zip(mrg.golden_names(case),
                                (retellings.WORK_FIELDS, retellings.PASSAGE_FIELDS), body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_input_holds_what_its_generator_says():
    rows = rt.read_rows(mrg.input_csv())
    names = [r[0] for r in rows]
    assert len(set(names)) == 12 and 200 <= len(rows) <= 400
    blocks = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
    assert len(blocks) > len(set(blocks))                      # a work comes back
    fans = {r[2] for r in rows}
    assert any("," in f for f in fans) and any('"' in f for f in fans)
    assert any(not f.isascii() for f in fans)
    made = mrg.build()
    works = {r.split(",")[0]: r.split(",") for r in
             made[mrg.golden_names("gap1_min1")[0]].split("\r\n")[1:-1]}
    assert set(works) == set(names) - {"d.txt"}                # d.txt has no passage
    assert works["a.txt"][1:7] == ["6", "43", "6", "43", "100", "0"]      # the clean retelling
    assert works["b.txt"][3] == "3" and works["b.txt"][6] == "3"          # the same lines scrambled
    assert works["dir/c.txt"][6] == "1"                                   # a repeated line
    assert works["f.txt"][3] == "1" and works["e.txt"][1] == "1"
    default = made[mrg.golden_names("default")[0]]
    assert "g.txt" not in default and "g.txt" in made[mrg.golden_names("gap1_min1")[0]]
    share = [r.split(",")[0] for r in made[mrg.golden_names("share80")[0]].split("\r\n")[1:-1]]
    assert share == ["a.txt", "j.txt", "i.txt", "k.txt"]
    assert '"4 > 7, later > 9 > 12 > 15"' in default           # scene 12 twice, written once
