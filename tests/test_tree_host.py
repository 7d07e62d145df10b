"""`ao3.py tree` without a GPU: the restated contract (tests/tree_restated.py) on examples worked
by hand, the parser, the refusals, the C ABI's declarations and the committed expected CSVs."""

import csv
import ctypes as C
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, tree
from tests import tree_restated as tr
from tests.golden import make_tree_golden as mtg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def records_of(spans_of):
    """Records (work, fan_ix, orig_ix) of works given as lists of (first script word, words)."""
    recs = []
    for w, spans in enumerate(spans_of):
        f = 0
        for o0, k in spans:
            recs += [(w, f + i, o0 + i) for i in range(k)]
            f += k + 10
    return recs


def run(spans_of, n_script=100, **kw):
    kw.setdefault("min_words", 1)
    kw.setdefault("min_shared", 1)
    return tr.tree(records_of(spans_of), len(spans_of), n_script, **kw)


def keys(rows, *names):
    return [tuple(r[n] for n in names) for r in rows]


# ---- the restatement on examples worked by hand --------------------------------------------

def test_levels_of_both_measures():
    assert tr.level_of("jaccard", 8, 15, 15) == 363636          # 8 of 22
    assert tr.level_of("jaccard", 7, 7, 7) == 1000000
    assert tr.level_of("jaccard", 1, 1 << 19, (1 << 19) + 1) == 0    # 1 of 2^20: below a part
    assert tr.level_of("jaccard", 1, 3, 1) == 333333            # rounded down
    assert tr.level_of("shared", 8, 15, 15) == 8
    with pytest.raises(ValueError):
        tr.level_of("cosine", 1, 1, 1)


def test_three_works_in_a_row():
    # 0 covers 0..9, 1 covers 5..14, 2 covers 12..21: 0-1 share 5 of 15, 1-2 share 3 of 17
    works, merges, levels = run([[(0, 10)], [(5, 10)], [(12, 10)]])
    assert keys(merges, "a", "b", "level", "shared", "left", "right", "left_works",
                "right_works", "works", "first_work", "tree", "run_first", "run_words") == [
        (0, 1, 333333, 5, NONE, NONE, 1, 1, 2, 0, 0, 5, 5),
        (1, 2, 176470, 3, 0, NONE, 2, 1, 3, 0, 0, 12, 3)]
    assert keys(works, "covered", "tree", "tree_works", "edges", "joined_merge", "joined_level",
                "best", "leaf") == [(10, 0, 3, 1, 0, 333333, 1, 0), (10, 0, 3, 2, 0, 333333, 0, 1),
                                    (10, 0, 3, 1, 1, 176470, 1, 2)]
    assert keys(levels, "level", "merges", "merges_above", "families", "largest", "joined",
                "singles") == [(333333, 1, 0, 1, 2, 2, 1), (176470, 1, 1, 1, 3, 3, 0)]
    # under --measure shared the same forest at levels 5 and 3
    assert keys(run([[(0, 10)], [(5, 10)], [(12, 10)]], measure="shared")[1], "level") == \
        [(5,), (3,)]


def test_the_right_side_may_be_the_earlier_family():
    # 1 and 2 merge first; then 0 joins through its edge to 2: left is work 0 alone, right the
    # family of 1 and 2, and the leaves are 0, 1, 2
    works, merges, _ = run([[(0, 4), (20, 2)], [(10, 8)], [(10, 8), (20, 2)]], measure="shared")
    assert keys(merges, "a", "b", "level", "left", "right", "left_works", "right_works") == [
        (1, 2, 8, NONE, NONE, 1, 1), (0, 2, 2, NONE, 0, 1, 2)]
    assert [w["leaf"] for w in works] == [0, 1, 2]
    assert [w["best"] for w in works] == [2, 2, 1]


def test_a_triangle_of_ties_keeps_the_two_earliest_edges():
    # three identical works: (0, 1), (0, 2) and (1, 2) tie; the third closes a cycle
    works, merges, levels = run([[(0, 6)]] * 3)
    assert keys(merges, "a", "b", "level", "left", "right") == [
        (0, 1, 1000000, NONE, NONE), (0, 2, 1000000, 0, NONE)]
    assert [w["edges"] for w in works] == [2, 1, 1]
    assert keys(levels, "level", "merges", "families", "largest", "singles") == \
        [(1000000, 2, 1, 3, 0)]


def test_equal_levels_go_by_a_then_b_across_pairs():
    # 0-3 and 1-2 both share 4 of 8; 0-1 and 2-3 nothing: (0, 3) comes before (1, 2)
    works, merges, _ = run([[(0, 6)], [(10, 6)], [(12, 6)], [(2, 6)]])
    assert keys(merges, "a", "b", "level") == [(0, 3, 500000), (1, 2, 500000)]
    # two trees of two: the one with the earlier work is ranked first
    assert [w["tree"] for w in works] == [0, 1, 1, 0]
    assert [w["leaf"] for w in works] == [0, 2, 3, 1]


def test_trees_are_ranked_by_size_and_a_lone_work_is_a_tree():
    spans = [[(0, 6)], [(50, 6)], [(20, 6)], [(20, 6)], [(20, 6)], [], [(0, 6)]]
    works, merges, levels = run(spans)
    assert [w["tree"] for w in works] == [1, 2, 0, 0, 0, NONE, 1]
    assert [w["tree_works"] for w in works] == [2, 1, 3, 3, 3, 0, 2]
    assert [w["leaf"] for w in works] == [3, 5, 0, 1, 2, NONE, 4]
    assert works[1]["joined_merge"] == NONE and works[1]["best"] == NONE
    assert works[5] == dict(covered=0, tree=NONE, tree_works=0, edges=0, joined_merge=NONE,
                            joined_level=0, best=NONE, leaf=NONE)
    assert [m["tree"] for m in merges] == [1, 0, 0]
    assert levels[-1]["singles"] == 1 and levels[-1]["families"] == 2


def test_min_shared_and_min_level_at_and_above_an_edge():
    spans = [[(0, 10)], [(5, 10)], [(12, 10)]]
    assert len(run(spans, min_shared=3)[1]) == 2 and len(run(spans, min_shared=4)[1]) == 1
    assert len(run(spans, min_level=176470)[1]) == 2 and len(run(spans, min_level=176471)[1]) == 1
    assert len(run(spans, measure="shared", min_level=5)[1]) == 1
    assert run(spans, measure="shared", min_level=6)[1] == []


def test_a_short_run_is_no_passage_and_a_bridged_word_is_covered():
    recs = records_of([[(0, 8)], [(0, 8)]])
    recs = [r for r in recs if r[:2] != (1, 4)]                  # work 1 steps over word 4
    assert tr.tree(recs, 2, 20, min_words=4, min_shared=1)[1][0]["shared"] == 4
    assert tr.tree(recs, 2, 20, min_words=5, min_shared=1)[1] == []
    works, merges, _ = tr.tree(recs, 2, 20, min_words=5, max_gap=1, min_shared=1)
    assert merges[0]["shared"] == 8 and works[1]["covered"] == 8


def test_refusals_of_the_restatement():
    recs = records_of([[(0, 8)], [(0, 8)]])
    for kw in (dict(min_words=0), dict(min_shared=0), dict(measure="cosine"),
               dict(min_level=-1), dict(min_level=1000001), dict(max_gap=-1)):
        with pytest.raises(ValueError):
            tr.tree(recs, 2, 20, **kw)
    tr.tree(recs, 2, 20, measure="shared", min_level=1000001)
    with pytest.raises(ValueError):
        tr.tree(recs, 1, 20)
    with pytest.raises(ValueError):
        tr.tree(recs, 2, 7)
    with pytest.raises(ValueError):
        tr.tree(recs[::-1], 2, 20)


# ---- the parser ----------------------------------------------------------------------------

def test_parser_defaults_and_options():
    args = cli.ao3_parser().parse_args(["tree", "runs/m.csv"])
    assert (args.min_words, args.max_gap, args.measure, args.min_shared, args.min_level,
            args.device, args.reader, args.output) == (6, 0, "jaccard", 6, 0, 0, None, None)
    assert tree.output_names(args.matches, args.output) == (
        "runs/m-tree.csv", "runs/m-tree-works.csv", "runs/m-tree-levels.csv")
    args = cli.ao3_parser().parse_args(
        ["tree", "m.csv", "-o", "out/x", "--measure", "shared", "--min-shared", "2",
         "--min-level", "7", "--min-words", "4", "--max-gap", "1", "--device", "1", "--reader",
         "python"])
    assert (args.min_words, args.max_gap, args.measure, args.min_shared, args.min_level,
            args.device, args.reader) == (4, 1, "shared", 2, 7, 1, "python")
    assert tree.output_names(args.matches, args.output) == (
        "out/x-tree.csv", "out/x-tree-works.csv", "out/x-tree-levels.csv")
    assert tree.output_names("m.txt") == ("m.txt-tree.csv", "m.txt-tree-works.csv",
                                          "m.txt-tree-levels.csv")
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["tree", "m.csv", "--measure", "cosine"])
    text = " ".join(cli.ao3_parser().format_help().split())
    assert "misquotes, tree, contrast" in text
    assert tree.MERGE_FIELDS == tr.MERGE_FIELDS and tree.WORK_FIELDS == tr.WORK_FIELDS and \
        tree.LEVEL_FIELDS == tr.LEVEL_FIELDS
    assert abi.TREE_MEASURES == tr.MEASURES


def test_the_pinned_parsers_do_not_know_the_command():
    for parser in (cli.build_parser(), cli.full_parser()):
        with pytest.raises(SystemExit):
            parser.parse_args(["tree", "m.csv"])


LEVEL_MESSAGE = "--min-level must be at least 0, and at most 1000000 under --measure jaccard"


@pytest.mark.parametrize("bad,message", [
    (["--min-shared", "0"], "--min-shared must be at least 1"),
    (["--min-level", "-1"], LEVEL_MESSAGE),
    (["--min-level", "1000001"], LEVEL_MESSAGE),
    (["--measure", "shared", "--min-level", "-1"], LEVEL_MESSAGE),
    (["--measure", "shared", "--min-level", str(1 << 32)], "--min-level must be below 2^32"),
    (["--min-words", "0"], "--min-words must be at least 1, --max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words must be at least 1, --max-gap at least 0")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["tree", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py tree: error: " + message


# ---- the C ABI -----------------------------------------------------------------------------

def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_tree", "fs_tree_rows", "fs_tree_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "tree" in _lib.TIMED
    assert abi.TREE_MS_NAMES == ("cover", "flatten", "best", "choose", "hook", "detail", "replay",
                                 "total", "rounds")
    assert re.search(r"#define FS_TREE_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_TREE_ROW_BYTES 60u", text)
    assert re.search(r"#define FS_TREE_MAX_ROUNDS 40u", text)
    assert re.search(r"#define FS_TREE_JACCARD 0u", text) and re.search(
        r"#define FS_TREE_SHARED 1u", text)
    assert (abi.FS_TREE_MAX_BYTES, abi.FS_TREE_ROW_BYTES, abi.FS_TREE_MAX_ROUNDS,
            abi.FS_TREE_JACCARD, abi.FS_TREE_SHARED) == (1 << 30, 60, 40, 0, 1)
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    body = open(os.path.join(src, "fs_tree.hip")).read()
    # the product, the union-find and the shared run are the shared ones, not copies
    assert '#include "fs_tiles.h"' in body and '#include "fs_unionfind.h"' in body
    assert "tile_counts(" in body and "uf_unite(" in body and "shared_run(" in body
    assert "uf_unite(uint32_t" not in body and "asm" not in body
    assert "uf_unite(uint32_t" not in open(os.path.join(src, "fs_clusters.hip")).read()
    assert "shared_run(" in open(os.path.join(src, "fs_pairs.hip")).read()
    make = open(os.path.join(src, "Makefile")).read()
    assert "fs_tree.hip" in make and "fs_unionfind.h" in make


@pytest.mark.parametrize("struct,dtype,keys,reserved,size", [
    ("fs_tree_merge", "TREE_MERGE_DTYPE", tr.MERGE_KEYS, ["reserved"], 64),
    ("fs_tree_work", "TREE_WORK_DTYPE", tr.WORK_KEYS, [], 32),
    ("fs_tree_level", "TREE_LEVEL_DTYPE", tr.LEVEL_KEYS, ["reserved"], 32)])
def test_dtypes_match_the_header(struct, dtype, keys, reserved, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for names in re.findall(r"\buint32_t\s+([^;]+);", body)
              for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == 4 * len(fields)
    assert list(dt.names) == fields == keys + reserved
    assert all(dt.fields[n] == (np.dtype(np.uint32), 4 * k) for k, n in enumerate(fields))


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    works = np.ones(2, dtype=abi.TREE_WORK_DTYPE)
    wp = works.ctypes.data_as(C.c_void_p)
    n_m, n_l = C.c_uint64(7), C.c_uint64(7)

    def call(n_rows=1, n_works=2, n_script=4, min_words=1, max_gap=0, measure=0, min_shared=1,
             min_level=0, works=wp, cap_m=0, cap_l=0, got_m=C.byref(n_m), got_l=C.byref(n_l),
             cols=u32):
        return L.fs_tree(0, cols, cols, cols, n_rows, n_works, n_script, min_words, max_gap,
                         measure, min_shared, min_level, works, None, cap_m, got_m, None, cap_l,
                         got_l)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    for bad in (dict(min_words=0), dict(min_shared=0), dict(measure=2), dict(min_level=1000001),
                dict(works=None), dict(cap_m=1), dict(cap_l=1), dict(got_m=None),
                dict(got_l=None)):
        assert call(**bad) == abi.FS_E_INVALID, bad
    assert (works["edges"] == 1).all()                                   # nothing written
    # no records: works without coverage, without device work
    assert call(n_rows=0, measure=1, min_level=1000001) == abi.FS_OK
    assert (n_m.value, n_l.value) == (0, 0)
    assert works.tolist() == [(0, NONE, 0, 0, NONE, 0, NONE, NONE)] * 2
    assert L.fs_tree_times(None) == abi.FS_E_INVALID
    ms = (C.c_double * 9)()
    assert L.fs_tree_times(ms) == abi.FS_OK and not any(ms)
    with pytest.raises(ValueError):
        tree.find_tree(z, z, z[:3], 2, 5)
    with pytest.raises(ValueError):
        tree.find_tree(z, z, z, 2, 5, measure="cosine")


# ---- the committed expected files ----------------------------------------------------------

def test_goldens_are_what_the_generator_writes():
    built = mtg.build()
    assert len(built) == 1 + 3 * len(mtg.CASES) == 10
    for name, text in built.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,options,kw", mtg.CASES)
def test_the_options_are_the_keywords(case, options, kw):
    args = cli.ao3_parser().parse_args(["tree", "m.csv"] + options)
    got = dict(min_words=args.min_words, max_gap=args.max_gap, measure=args.measure,
               min_shared=args.min_shared, min_level=args.min_level)
    assert {k: got[k] for k in kw} == kw


def test_the_cases_the_issue_names():
    assert [c[1] for c in mtg.CASES] == [
        [], ["--measure", "shared", "--min-shared", "2"],
        ["--max-gap", "1", "--min-words", "4", "--min-level", "300000"]]


def test_what_the_golden_input_holds():
    def rows(case, kind):
        name = mtg.golden_names(case)[mtg.KINDS.index(kind)]
        with open(os.path.join(GOLDEN, name), newline="", encoding="utf-8") as fh:
            return list(csv.DictReader(fh))
    merges = rows("defaults", "tree")
    works = {r["FAN_WORK_FILENAME"]: r for r in rows("defaults", "works")}
    assert len(works) == 10 and "j.txt" not in works and "k.txt" not in works
    # two works of identical coverage: the first merge, at a million
    first = merges[0]
    assert (first["A_FAN_WORK_FILENAME"], first["B_FAN_WORK_FILENAME"], first["LEVEL"],
            first["SHARED_WORDS"], first["A_COVERED_WORDS"], first["B_COVERED_WORDS"]) == \
        ("a.txt", "b.txt", "1000000", "15", "15", "15")
    # the tie of d.txt's three edges: the one from a.txt is the merge
    last = merges[-1]
    assert (last["LEVEL"], last["A_FAN_WORK_FILENAME"], last["B_FAN_WORK_FILENAME"]) == \
        ("318181", "a.txt", "d.txt")
    assert tr.level_of("jaccard", 7, 15, 14) == tr.level_of("jaccard", 7, 14, 15) == 318181
    # a work that joins nothing, and two separate trees, the larger and later one first
    assert (works["i.txt"]["TREE"], works["i.txt"]["TREE_WORKS"], works["i.txt"]["EDGES"],
            works["i.txt"]["JOINED_AT_MERGE"], works["i.txt"]["BEST_PARTNER"]) == \
        ("3", "1", "0", "", "")
    assert {works[n]["TREE"] for n in ("a.txt", "b.txt", "dir/c.txt", "d.txt")} == {"2"}
    assert {works[n]["TREE"] for n in ("e.txt", "f.txt", "g.txt", "h.txt", "l.txt")} == {"1"}
    assert sorted(int(w["LEAF_ORDER"]) for w in works.values()) == list(range(10))
    assert [n for n, w in sorted(works.items(), key=lambda t: int(t[1]["LEAF_ORDER"]))][:5] == \
        ["e.txt", "f.txt", "h.txt", "g.txt", "l.txt"]
    levels = rows("defaults", "levels")
    assert [r["LEVEL"] for r in levels] == sorted({m["LEVEL"] for m in merges}, key=int,
                                                  reverse=True)
    assert (levels[-1]["FAMILIES"], levels[-1]["LARGEST_WORKS"], levels[-1]["SINGLE_WORKS"]) == \
        ("2", "5", "1")
    assert sum(int(r["MERGES"]) for r in levels) == len(merges) == 7
    # under --measure shared three merges tie at eight words, across the trees
    shared = rows("shared_s2", "tree")
    assert [(m["A_FAN_WORK_FILENAME"], m["B_FAN_WORK_FILENAME"]) for m in shared
            if m["LEVEL"] == "8"] == [("a.txt", "dir/c.txt"), ("e.txt", "g.txt"),
                                      ("e.txt", "l.txt")]
    # --max-gap 1 --min-words 4: j.txt and k.txt have passages; --min-level 300000 drops
    # e.txt -- h.txt, and h.txt joins through f.txt
    gap = rows("gap1_words4_level300000", "tree")
    gworks = {r["FAN_WORK_FILENAME"]: r for r in rows("gap1_words4_level300000", "works")}
    assert gworks["k.txt"]["COVERED_WORDS"] == "8" and gworks["j.txt"]["EDGES"] == "0"
    assert gworks["h.txt"]["BEST_PARTNER"] == "f.txt" and gworks["h.txt"]["JOINED_AT_LEVEL"] == \
        "428571"
    assert [(m["A_FAN_WORK_FILENAME"], m["B_FAN_WORK_FILENAME"]) for m in gap
            if m["LEVEL"] == "533333"] == [("a.txt", "k.txt"), ("dir/c.txt", "k.txt")]
    assert all(int(m["LEVEL"]) >= 300000 for m in gap)
    # a file without records: three header rows
    from tests.passages_restated import MATCH_FIELDS
    assert tr.tree_csv(",".join(MATCH_FIELDS) + "\r\n") == tuple(
        ",".join(f) + "\r\n" for f in (tr.MERGE_FIELDS, tr.WORK_FIELDS, tr.LEVEL_FIELDS))
