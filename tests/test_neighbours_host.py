"""`ao3.py neighbours` without a GPU: the restated contract (tests/neighbours_restated.py) on
examples worked by hand, the parser, the refusals, the C ABI's declarations and the committed
expected CSVs."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, neighbours
from tests import neighbours_restated as nr
from tests.golden import make_neighbours_golden as mng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def records_of(spans_of):
    """Records of works given as lists of (first script word, words): a diagonal run per span,
    the fan index jumping between them."""
    recs = []
    for w, spans in enumerate(spans_of):
        f = 0
        for o0, k in spans:
            recs += [(w, f + i, o0 + i) for i in range(k)]
            f += k + 10
    return recs


def listed(found, a):
    return [(p["b"], p["ppm"]) for p in found if p["a"] == a]


# ---- the restatement on examples worked by hand --------------------------------------------

def test_weight_rule_at_its_bounds():
    for n in (1, 2, 7, 8, 9, 31244):
        assert nr.weight_of(n, 0) == 0 and nr.weight_of(n, 0, "flat") == 0
        assert nr.weight_of(n, n) == 1                       # every work covers it
        assert nr.weight_of(n, n // 2 + 1) == 1              # more than half of them
        assert nr.weight_of(n, 1) == n.bit_length()          # one work
        assert all(nr.weight_of(n, d, "flat") == 1 for d in range(1, n + 1))
        assert all(1 <= nr.weight_of(n, d) <= 32 for d in range(1, min(n, 100) + 1))
    assert nr.weight_of(1, 1) == 1                           # N = 1
    # N = 8, a power of two: exactly half the works is weight 2, one work 4
    assert [nr.weight_of(8, d) for d in range(1, 9)] == [4, 3, 2, 2, 1, 1, 1, 1]
    # N = 7, one below: 7 // 3 = 2, two bits; one work 3
    assert [nr.weight_of(7, d) for d in range(1, 8)] == [3, 2, 2, 1, 1, 1, 1]
    assert nr.weight_of(31244, 31244 // 2) == 2
    assert nr.weight_of(2 ** 32 - 1, 1) == 32                # the largest there is
    with pytest.raises(ValueError):
        nr.weight_of(4, 1, "idf")


def test_one_active_work_has_no_neighbours():
    works, words, found = nr.neighbours(records_of([[(0, 6)], [(3, 2)]]), 2, 10)
    assert found == []
    assert works[0] == dict(covered=6, own=6, candidates=0, listed=0, listed_by=0, mutual=0,
                            nearest=NONE, nearest_ppm=0)
    assert works[1]["covered"] == 0 and works[1]["nearest"] == NONE
    assert [w["depth"] for w in words] == [1] * 6 + [0] * 4
    assert [w["weight"] for w in words] == [1] * 6 + [0] * 4          # N = 1: one bit


def test_two_identical_works_are_mutual_at_rank_one():
    works, words, found = nr.neighbours(records_of([[(2, 8)], [(2, 8)]]), 2, 12)
    # N = 2, depth 2: weight 1; own = score = 8
    assert found == [dict(a=0, b=1, rank=1, back_rank=1, ppm=1000000, score=8, shared=8,
                          rarest=2, rarest_depth=2, rarest_weight=1, run_first=2, run_words=8),
                     dict(a=1, b=0, rank=1, back_rank=1, ppm=1000000, score=8, shared=8,
                          rarest=2, rarest_depth=2, rarest_weight=1, run_first=2, run_words=8)]
    assert all(w == dict(covered=8, own=8, candidates=1, listed=1, listed_by=1, mutual=1,
                         nearest=1 - k, nearest_ppm=1000000) for k, w in enumerate(works))
    assert list(found[0]) == nr.NEIGHBOUR_KEYS and list(works[0]) == nr.WORK_KEYS
    assert list(words[0]) == nr.WORD_KEYS


def test_a_tie_goes_to_the_earlier_work_and_top_may_exceed_the_candidates():
    # works 1 and 2 are copies: both are as close to work 0, and to work 3
    spans = [[(0, 6), (10, 6)], [(0, 6), (20, 6)], [(0, 6), (20, 6)], [(20, 6), (30, 6)]]
    works, words, found = nr.neighbours(records_of(spans), 4, 40, top=32)
    at0, at3 = listed(found, 0), listed(found, 3)
    assert [b for b, _ in at0] == [1, 2] and at0[0][1] == at0[1][1]
    assert [b for b, _ in at3] == [1, 2] and at3[0][1] == at3[1][1]
    assert [w["candidates"] for w in works] == [2, 3, 3, 2]          # 0 and 3 share nothing
    assert [w["listed"] for w in works] == [2, 3, 3, 2]              # top 32: all of them
    assert [b for b, _ in listed(found, 1)] == [2, 0, 3] or \
        [b for b, _ in listed(found, 1)] == [2, 3, 0]
    # with room for one the earlier of the two is listed, and the later one is not listed back
    works, words, found = nr.neighbours(records_of(spans), 4, 40, top=1)
    assert listed(found, 0)[0][0] == 1 and listed(found, 3)[0][0] == 1
    assert [w["candidates"] for w in works] == [2, 3, 3, 2]
    assert [w["listed_by"] for w in works] == [0, 3, 1, 0]
    by = {p["a"]: p for p in found}
    assert (by[1]["b"], by[1]["back_rank"], by[2]["b"], by[2]["back_rank"]) == (2, 1, 1, 1)
    assert by[0]["back_rank"] == NONE and [w["mutual"] for w in works] == [0, 1, 1, 0]


def test_min_similarity_exactly_at_its_bound():
    # flat: work 1 covers half of what work 0 covers and nothing else: 3 / (6 + 3 - 3)
    spans = [[(0, 6)], [(0, 3)]]
    for bound, kept in ((49, True), (50, True), (51, False)):
        works, _, found = nr.neighbours(records_of(spans), 2, 6, min_words=3, weight="flat",
                                        min_similarity=bound)
        assert [p["ppm"] for p in found] == ([500000, 500000] if kept else [])
        assert works[0]["candidates"] == int(kept)
    # and min_score at its bound: the score is 3
    assert len(nr.neighbours(records_of(spans), 2, 6, min_words=3, weight="flat",
                             min_score=3)[2]) == 2
    assert nr.neighbours(records_of(spans), 2, 6, min_words=3, weight="flat",
                         min_score=4)[2] == []


def test_a_popular_line_ranks_below_a_rare_one():
    """Six works of two lines each.  Line P (words 0-5) is quoted by five of them, line R
    (10-15) by works 0 and 1, every other line by one work.  N = 6: P weighs 1 (6 // 5 = 1), R
    weighs 2 (6 // 2 = 3), the others 3 (6 // 1 = 6)."""
    spans = [[(0, 6), (10, 6)], [(10, 6), (20, 6)], [(0, 6), (30, 6)], [(0, 6), (40, 6)],
             [(0, 6), (50, 6)], [(0, 6), (60, 6)]]
    works, words, found = nr.neighbours(records_of(spans), 6, 70)
    assert [words[o]["weight"] for o in (0, 10, 20, 30)] == [1, 2, 3, 3]
    assert [w["own"] for w in works] == [18, 30, 24, 24, 24, 24]
    # work 1 shares R: 12 / (18 + 30 - 12); works 2 .. 5 share P: 6 / (18 + 24 - 6)
    assert listed(found, 0) == [(1, 333333), (2, 166666), (3, 166666), (4, 166666),
                                (5, 166666)]
    first = [p for p in found if p["a"] == 0][0]
    assert (first["rarest"], first["rarest_weight"], first["rarest_depth"]) == (10, 2, 2)
    # flat: six shared words either way, 6 / (12 + 12 - 6): the two tie, the earlier first
    works, words, found = nr.neighbours(records_of(spans), 6, 70, weight="flat")
    assert listed(found, 0) == [(b, 333333) for b in (1, 2, 3, 4, 5)]


def test_the_run_is_the_one_holding_the_rarest_word():
    """Works 0 and 1 share ten words of a line works 2 and 3 quote too, and three words nobody
    else has: the run is the three words, not the longer one."""
    spans = [[(0, 10), (20, 3)], [(0, 10), (19, 5)], [(0, 10)], [(0, 12)]]
    works, words, found = nr.neighbours(records_of(spans), 4, 30, min_words=3)
    p = [p for p in found if (p["a"], p["b"]) == (0, 1)][0]
    assert (p["shared"], p["rarest"], p["run_first"], p["run_words"]) == (13, 20, 20, 3)
    assert (p["rarest_depth"], p["rarest_weight"]) == (2, 2)         # 4 // 2 = 2: two bits
    assert p["score"] == 10 * 1 + 3 * 2
    # among equals the first: works 2 and 3 share ten words of weight 1
    q = [p for p in found if (p["a"], p["b"]) == (2, 3)][0]
    assert (q["rarest"], q["run_first"], q["run_words"], q["rarest_weight"]) == (0, 0, 10, 1)
    assert nr.run_around({1, 2, 3, 5, 6}, 5) == (5, 2)
    assert nr.run_around({1, 2, 3, 5, 6}, 2) == (1, 3)


def test_restatement_refuses_what_the_library_refuses():
    recs = records_of([[(0, 6)]])
    for kw in (dict(top=0), dict(top=33), dict(min_score=0), dict(min_similarity=101),
               dict(min_words=0), dict(weight="idf")):
        with pytest.raises(ValueError):
            nr.neighbours(recs, 1, 6, **kw)
    with pytest.raises(ValueError):
        nr.neighbours(recs, 1, 5)


# ---- product side that needs no GPU -------------------------------------------------------

def test_field_lists_are_the_restatement_s():
    assert neighbours.NEIGHBOUR_FIELDS == nr.NEIGHBOUR_FIELDS
    assert neighbours.WORK_FIELDS == nr.WORK_FIELDS
    assert neighbours.WORD_FIELDS == nr.WORD_FIELDS
    assert list(abi.NEIGHBOUR_DTYPE.names) == nr.NEIGHBOUR_KEYS
    assert list(abi.NEIGHBOUR_WORK_DTYPE.names) == nr.WORK_KEYS
    assert list(abi.NEIGHBOUR_WORD_DTYPE.names) == nr.WORD_KEYS


def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["neighbours", "runs/m.csv"])
    assert args.func.__name__ == "_neighbours"
    assert (args.output, args.weight, args.top, args.min_score, args.min_similarity,
            args.min_words, args.max_gap, args.device, args.reader) == \
        (None, "rarity", 10, 1, 0, 6, 0, 0, None)
    assert neighbours.output_names(args.matches) == (
        "runs/m-neighbours.csv", "runs/m-neighbours-works.csv", "runs/m-neighbours-words.csv")
    assert neighbours.output_names("m.csv", "out/x")[2] == "out/x-neighbours-words.csv"
    args = cli.ao3_parser().parse_args(
        ["neighbours", "m.csv", "-o", "p", "--weight", "flat", "--top", "32", "--min-score", "4",
         "--min-similarity", "100", "--min-words", "3", "--max-gap", "2", "--device", "1",
         "--reader", "python"])
    assert (args.output, args.weight, args.top, args.min_score, args.min_similarity,
            args.min_words, args.max_gap, args.device, args.reader) == \
        ("p", "flat", 32, 4, 100, 3, 2, 1, "python")
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["neighbours", "m.csv", "--weight", "idf"])
    assert "neighbours" in cli.ao3_parser().format_help()
    assert "neighbours" not in cli.full_parser().format_help()
    assert neighbours.WEIGHT == ("rarity", "flat")
    assert "neighbours" in _lib.TIMED


@pytest.mark.parametrize("bad,message", [
    (["--top", "0"], "--top must be from 1 to 32"),
    (["--top", "33"], "--top must be from 1 to 32"),
    (["--min-score", "0"], "--min-score must be at least 1"),
    (["--min-similarity", "101"], "--min-similarity must be from 0 to 100"),
    (["--min-similarity", "-1"], "--min-similarity must be from 0 to 100"),
    (["--min-words", "0"], "--min-words must be at least 1, --max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words must be at least 1, --max-gap at least 0")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["neighbours", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py neighbours: error: " + message


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_neighbours", "fs_neighbours_rows", "fs_neighbours_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.NEIGHBOURS_MS_NAMES == ("coverage", "weights", "product", "place", "detail",
                                       "total")
    assert re.search(r"#define FS_NEIGHBOURS_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_NEIGHBOURS_MAX_TOP 32u", text)
    assert (abi.FS_NEIGHBOURS_MAX_BYTES, abi.FS_NEIGHBOURS_MAX_TOP, abi.FS_NEIGHBOURS_RARITY,
            abi.FS_NEIGHBOURS_FLAT) == (1 << 30, 32, 0, 1) and nr.MAX_TOP == 32
    # the product is the matrix instruction, the scans and reductions the shared ones
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    body = open(os.path.join(src, "fs_neighbours.hip")).read()
    assert "__builtin_amdgcn_mfma_i32_16x16x64_i8" in body and "asm" not in body
    assert '#include "fs_tiles.h"' in body and "RowsSrc" in open(
        os.path.join(src, "fs_tiles.h")).read()
    assert "__shfl_xor" not in body and "fs_host_rows(" in body
    assert "fs_neighbours.hip" in open(os.path.join(src, "Makefile")).read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_neighbour", "NEIGHBOUR_DTYPE", nr.NEIGHBOUR_KEYS, 48),
    ("fs_neighbour_work", "NEIGHBOUR_WORK_DTYPE", nr.WORK_KEYS, 32),
    ("fs_neighbour_word", "NEIGHBOUR_WORD_DTYPE", nr.WORD_KEYS, 8)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for names in re.findall(r"\buint32_t\s+([^;]+);", body)
              for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == 4 * len(fields)
    assert list(dt.names) == fields == keys
    assert all(dt.fields[n] == (np.dtype(np.uint32), 4 * k) for k, n in enumerate(fields))


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    works = np.ones(2, dtype=abi.NEIGHBOUR_WORK_DTYPE)
    words = np.ones(4, dtype=abi.NEIGHBOUR_WORD_DTYPE)
    wp, op = works.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p)
    n = C.c_uint64(7)

    def call(n_rows=1, n_works=2, n_script=4, min_words=1, weight=0, top=10, min_score=1,
             min_similarity=0, works=wp, words=op, out=None, cap=0, got=C.byref(n), cols=u32):
        return L.fs_neighbours(0, cols, cols, cols, n_rows, n_works, n_script, min_words, 0,
                               weight, top, min_score, min_similarity, works, words, out, cap,
                               got)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_score=0) == abi.FS_E_INVALID
    for top in (0, 33):
        assert call(top=top) == abi.FS_E_INVALID
        assert b"from 1 to 32" in L.fs_last_error()
    assert call(min_similarity=101) == abi.FS_E_INVALID
    assert call(weight=2) == abi.FS_E_INVALID
    assert call(works=None) == abi.FS_E_INVALID
    assert call(words=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                        # room for a pair, no buffer
    assert call(got=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (works["own"] == 1).all() and (words["depth"] == 1).all()     # nothing written
    # no records: works without coverage and words without depth, without device work
    assert call(n_rows=0) == abi.FS_OK and n.value == 0
    assert works.tolist() == [(0, 0, 0, 0, 0, 0, NONE, 0)] * 2 and not words["depth"].any()
    assert L.fs_neighbours_times(None) == abi.FS_E_INVALID
    assert L.fs_neighbours_rows(None, None, 0, 0, 1, 0, 0, 10, 1, 0, None, None, None, 0,
                                C.byref(n)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        neighbours.find_neighbours(z, z, z[:3], 2, 4)
    with pytest.raises(ValueError):
        neighbours.find_neighbours(z, z, z, 2, 4, weight="idf")


# ---- the committed expected files ----------------------------------------------------------

@pytest.mark.parametrize("case,options,kw", mng.CASES)
def test_goldens_are_what_the_restatement_writes(case, options, kw):
    with open(os.path.join(GOLDEN, mng.INPUT), newline="", encoding="utf-8") as fh:
        want = nr.neighbours_csv(fh.read(), **kw)
    for name, text in zip(mng.golden_names(case), want):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name
    rows = want[0].count("\r\n") - 1
    assert rows > 0 and want[1].count("\r\n") - 1 == 8
    # the options are the keywords
    args = cli.ao3_parser().parse_args(["neighbours", "m.csv"] + options)
    got = dict(weight=args.weight, top=args.top, min_score=args.min_score,
               min_similarity=args.min_similarity, min_words=args.min_words,
               max_gap=args.max_gap)
    assert {k: got[k] for k in kw} == kw


def test_the_default_golden_has_several_weights_and_a_tie():
    import csv
    names = mng.golden_names("defaults")
    with open(os.path.join(GOLDEN, names[2]), newline="", encoding="utf-8") as fh:
        words = list(csv.DictReader(fh))
    assert len({r["WEIGHT"] for r in words}) >= 2
    with open(os.path.join(GOLDEN, names[0]), newline="", encoding="utf-8") as fh:
        rows = list(csv.DictReader(fh))
    ppm_of = {}
    for r in rows:
        ppm_of.setdefault(r["FAN_WORK_FILENAME"], []).append(r["SIMILARITY_PPM"])
    assert any(len(set(v)) < len(v) for v in ppm_of.values())
    # a file without records: three header rows
    from tests.passages_restated import MATCH_FIELDS
    assert nr.neighbours_csv(",".join(MATCH_FIELDS) + "\r\n") == tuple(
        ",".join(f) + "\r\n" for f in (nr.NEIGHBOUR_FIELDS, nr.WORK_FIELDS, nr.WORD_FIELDS))
