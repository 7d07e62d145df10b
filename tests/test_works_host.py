"""`ao3.py works` without a GPU: the oracle's known answers, the parser, the C ABI's
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
from tests import works_restated as wr
from tests.golden import make_works_golden as mwg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _rec(work, fan, orig, comb=0.0):
    return (work, fan, orig, 0.0, comb)


def _diag(work, fan0, orig0, n, comb=0.0):
    return [_rec(work, fan0 + k, orig0 + k, comb) for k in range(n)]


# ---- oracle known answers -------------------------------------------------------------

def test_one_work():
    recs = _diag(0, 5, 10, 8, comb=0.07) + [_rec(0, 20, 3, 0.0), _rec(0, 21, 30, 0.6)]
    group_of = [0] * 16 + [1] * 16
    out, counts, cells = wr.works(recs, 1, 32, group_of, 2, min_words=6)
    assert out == [dict(first=0, n_words=10, fan_first=5, fan_last=21, n_script_words=10,
                        n_passages=1, passage_words=8, longest=8, n_groups_hit=2, top_group=0,
                        top_group_words=7)]
    #              <=0  .05 .1 ...                      .5  all
    assert counts == [[1, 1, 9, 9, 9, 9, 9, 9, 9, 9, 9, 10]]
    assert cells == [(0, 0, 7, 1), (0, 1, 3, 0)]


def test_tie_for_the_top_group_takes_the_smallest_id():
    recs = [_rec(0, 0, 5), _rec(0, 1, 1), _rec(0, 2, 3), _rec(0, 3, 4), _rec(0, 4, 2), _rec(0, 5, 0)]
    out, _, cells = wr.works(recs, 1, 6, [2, 2, 1, 1, 0, 0], 3, min_words=1)
    assert (out[0]["top_group"], out[0]["top_group_words"], out[0]["n_groups_hit"]) == (0, 2, 3)
    assert cells == [(0, 0, 2, 2), (0, 1, 2, 2), (0, 2, 2, 2)]
    out, _, _ = wr.works(recs[1:5], 1, 6, [2, 2, 1, 1, 0, 0], 3, min_words=1)
    assert (out[0]["top_group"], out[0]["top_group_words"]) == (1, 2)


def test_repeated_script_word_counts_once():
    recs = [_rec(0, k, 7) for k in range(5)] + [_rec(0, 9, 8)]
    out, counts, cells = wr.works(recs, 1, 9, [0] * 9, 1, min_words=1)
    assert out[0]["n_script_words"] == 2 and out[0]["n_words"] == 6
    assert out[0]["n_passages"] == 6 and out[0]["longest"] == 1    # no run: the script stands still
    assert cells == [(0, 0, 6, 6)] and counts[0][-1] == 6


def test_nan_and_negative_zero():
    recs = [_rec(0, 0, 0, NAN), _rec(0, 1, 1, -0.0), _rec(0, 2, 2, 0.0), _rec(0, 3, 3, 0.05),
            _rec(0, 4, 4, 0.5), _rec(0, 5, 5, 0.51)]
    out, counts, cells = wr.works(recs, 1, 6, [0, 0, 0, 1, 1, 1], 2, min_words=6)
    assert counts == [[2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 4, 6]]          # NaN only in the last column
    assert cells == [(0, 0, 3, 2), (0, 1, 3, 0)]
    assert out[0]["n_passages"] == 1 and out[0]["top_group"] == 0


def test_empty_work_between_two_others():
    recs = _diag(0, 0, 0, 3) + _diag(2, 4, 1, 2)
    out, counts, cells = wr.works(recs, 4, 4, [0, 1, 1, 1], 2, min_words=2)
    assert [o["n_words"] for o in out] == [3, 0, 2, 0]
    assert [o["first"] for o in out] == [0, 0, 3, 0]
    assert [o["top_group"] for o in out] == [1, wr.NONE, 1, wr.NONE]
    assert out[1] == dict.fromkeys(wr.WORK_KEYS, 0) | dict(top_group=wr.NONE)
    assert counts[1] == [0] * 12 and counts[3] == [0] * 12
    assert cells == [(0, 0, 1, 1), (0, 1, 2, 2), (2, 1, 2, 2)]
    assert (out[2]["fan_first"], out[2]["fan_last"], out[2]["longest"]) == (4, 5, 2)


def test_without_a_map_there_are_no_groups():
    out, counts, cells = wr.works(_diag(0, 0, 0, 6), 1, 6, None, 0)
    assert cells == [] and out[0]["n_groups_hit"] == 0 and out[0]["top_group"] == wr.NONE
    assert out[0]["top_group_words"] == 0 and out[0]["n_script_words"] == 6


def test_refusals():
    ok = _diag(0, 0, 0, 3)
    for kw in (dict(min_words=0), dict(n_works=0), dict(n_script=2),
               dict(group_of=[0, 0, 1], n_groups=1)):
        args = dict(n_works=1, n_script=3, group_of=[0, 0, 0], n_groups=1, min_words=1)
        args.update(kw)
        with pytest.raises(ValueError):
            wr.works(ok, **args)
    with pytest.raises(ValueError):
        wr.works([_rec(0, 1, 0), _rec(0, 0, 1)], 1, 3, None, 0)
    assert wr.works([], 2, 0, None, 0)[1] == [[0] * 12] * 2


def _row(name, fan, orig, scene, char, comb="0.0"):
    return [name, fan, "f%d" % fan, 1, orig, "W%d" % orig, 2, char, scene, "0.0", 7, comb]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_labels_are_numbered_in_script_order():
    # the later scene "9" and the character "ZED" come first in the script
    rows = [_row("a.txt", 0, 50, "2", "ANNA"), _row("a.txt", 1, 51, "2", "ANNA"),
            _row("b.txt", 0, 7, "9", "ZED"), _row("b.txt", 1, 60, "2", "BOB"),
            _row("b.txt", 2, 8, "9", "ANNA", comb="0.2")]
    assert wr.label_groups([50, 51, 7, 60, 8], ["2", "2", "9", "2", "9"]) == \
        ([0] * 7 + [0, 0] + [0] * 41 + [1, 1] + [0] * 8 + [1], ["9", "2"])
    works, scenes, chars = wr.works_csv(_match_csv(rows), 2)
    assert works.split("\r\n")[1:] == [
        "a.txt,2,2" + ",2" * 11 + ",2,1,2,2,0,1,1,2,2,1,ANNA,2",
        "b.txt,3,2,2,2,2,2" + ",3" * 7 + ",3,0,0,0,0,2,2,9,2,3,ZED,1", ""]
    assert scenes.split("\r\n")[1:] == ["a.txt,2,2,2", "b.txt,9,2,1", "b.txt,2,1,1", ""]
    assert chars.split("\r\n")[1:] == ["a.txt,ANNA,2,2", "b.txt,ZED,1,1", "b.txt,ANNA,1,0",
                                       "b.txt,BOB,1,1", ""]
    assert wr.works_csv(_match_csv(rows, header=False), 2) == (works, scenes, chars)


def test_a_script_word_with_two_labels_is_an_error():
    from fandom_search_amd import works
    rows = [_row("a.txt", 0, 5, "1", "ANNA"), _row("a.txt", 1, 6, "1", "ANNA"),
            _row("b.txt", 0, 5, "4", "ANNA")]
    with pytest.raises(ValueError):
        wr.works_csv(_match_csv(rows))
    with pytest.raises(ValueError, match="script word 5 "):
        works.label_groups(np.array([5, 6, 5]), ["1", "1", "4"], "scene")
    group_of, names = works.label_groups(np.array([9, 2, 9]), ["b", "a", "b"], "scene")
    assert group_of.tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1] and names == ["a", "b"]


def test_empty_input():
    works, scenes, chars = wr.works_csv("")
    assert works == ",".join(wr.WORK_FIELDS) + "\r\n"
    assert scenes == ",".join(wr.SCENE_FIELDS) + "\r\n"
    assert chars == ",".join(wr.CHARACTER_FIELDS) + "\r\n"


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import works
    args = cli.build_parser().parse_args(["works", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_works"
    assert (args.output, args.min_words, args.max_gap, args.device) == (None, 6, 0, 0)
    assert works.output_names(args.matches) == ("runs/match-6gram-20240101-works.csv",
                                                "runs/match-6gram-20240101-works-scenes.csv",
                                                "runs/match-6gram-20240101-works-characters.csv")
    assert works.output_names("batch", None)[0] == "batch-works.csv"
    assert works.output_names("m.csv", "out/x")[2] == "out/x-works-characters.csv"
    args = cli.build_parser().parse_args(["works", "m.csv", "-o", "p", "--min-words", "3",
                                          "--max-gap", "2", "--device", "1"])
    assert (args.output, args.min_words, args.max_gap, args.device) == ("p", 3, 2, 1)
    assert works.WORK_FIELDS == wr.WORK_FIELDS
    assert works.SCENE_FIELDS == wr.SCENE_FIELDS
    assert works.CHARACTER_FIELDS == wr.CHARACTER_FIELDS
    assert list(works.THRESHOLDS) == wr.THRESHOLDS


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_works_entry_points():
    for name in ("fs_works", "fs_works_rows"):
        assert name in _declared_functions()
        assert name in _lib.SYMBOLS
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    assert hasattr(lib, "fs_works") and hasattr(lib, "fs_works_rows")


@pytest.mark.parametrize("struct,dtype,size", [("fs_work", "WORK_DTYPE", 56),
                                               ("fs_work_cell", "WORK_CELL_DTYPE", 16)])
def test_dtypes_match_the_header(struct, dtype, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(uint64_t|uint32_t|double)\s+([^;]+);", body):
        fields += [(n.strip(), ctype) for n in names.split(",")]
    width = {"uint64_t": 8, "uint32_t": 4, "double": 8}
    off, want = 0, []
    for n, t in fields:
        off = (off + width[t] - 1) // width[t] * width[t]
        want.append((n, off))
        off += width[t]
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == off
    assert [(n, dt.fields[n][1]) for n in dt.names] == want
    assert set(wr.WORK_KEYS) | {"reserved", "reserved2"} == set(abi.WORK_DTYPE.names)


def test_limits_match_the_header():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    assert re.search(r"#define FS_WORKS_MAX_SCRIPT \(1u << 19\)", text)
    assert re.search(r"#define FS_WORKS_MAX_GROUPS 4096u", text)
    assert (abi.FS_WORKS_MAX_SCRIPT, abi.FS_WORKS_MAX_GROUPS) == (1 << 19, 4096)


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    d = np.zeros(1, dtype=np.float64)
    thr = np.array(wr.THRESHOLDS)
    out = np.ones(2, dtype=abi.WORK_DTYPE)
    counts = np.ones((2, 12), dtype=np.uint32)
    u32, f64, t = abi.ptr(z, C.c_uint32), abi.ptr(d, C.c_double), abi.ptr(thr, C.c_double)
    o, c = out.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_works=2, n_script=4, group_of=u32, n_groups=1, min_words=6, thr=t,
             n_thr=11):
        return L.fs_works(0, u32, u32, u32, f64, n_rows, n_works, n_script, group_of, n_groups,
                          min_words, 0, thr, n_thr, o, c, None, 0, C.byref(n))
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1, n_groups=0, group_of=None) == abi.FS_E_UNSUPPORTED
    assert call(n_groups=4097) == abi.FS_E_UNSUPPORTED
    assert call(n_thr=0) == abi.FS_E_INVALID and call(n_thr=65) == abi.FS_E_INVALID
    down = np.array([0.5, 0.1])
    assert call(thr=abi.ptr(down, C.c_double), n_thr=2) == abi.FS_E_INVALID
    assert call(n_groups=1, group_of=None) == abi.FS_E_INVALID
    bad = np.array([0, 0, 1, 0], dtype=np.uint32)
    assert call(group_of=abi.ptr(bad, C.c_uint32)) == abi.FS_E_INVALID
    assert b"group_of[2]" in L.fs_last_error()
    # no records: empty summaries without device work
    assert call(n_rows=0) == abi.FS_OK and n.value == 0
    assert (out["top_group"] == wr.NONE).all() and not out["n_words"].any() and not counts.any()
    assert L.fs_works_rows(None, None, 0, 0, None, 0, 6, 0, t, 11, None, None, None, 0,
                           C.byref(n)) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

@pytest.mark.parametrize("case,src,m,g", mwg.CASES)
def test_golden_files_are_the_oracle_output(case, src, m, g):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    got = wr.works_csv(text, m, g)
    for name, part in zip(mwg.golden_names(case, m, g), got):
        with open(os.path.join(gold, name), newline="", encoding="utf-8") as fh:
            want = fh.read()
        assert part == want, name
        assert want.count("\r\n") > 1                   # every case has works and cells
