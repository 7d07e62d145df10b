"""`ao3.py transitions` without a GPU: the oracle's known answers worked by hand
(tests/transitions_restated.py), the keep rule at its bounds, the host arithmetic of the two
files, the parser, the C ABI's declarations, and the committed expected CSVs under the product's
table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, transitions
from fandom_search_amd.passages import read_matches
from tests import companions_restated as cr
from tests import transitions_restated as tr
from tests.golden import make_transitions_golden as mtg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def placed(works, words=2):
    """Records (work, fan_ix, orig_ix) of works given as lists of (first fan word, first script
    word), passages of `words` words."""
    return [(w, fan + k, orig + k) for w, spans in enumerate(works) for fan, orig in spans
            for k in range(words)]


def cells_of(found):
    return {(c["a"], c["b"]): (c["steps"], c["advances"], c["works"], c["first_work"])
            for c in found}


# ---- oracle known answers, worked by hand ------------------------------------------------

UNIT_OF = [0] * 10 + [1] * 10 + [2] * 10 + [NONE] * 10
HAND = placed([[(0, 0), (5, 10), (10, 0), (20, 10)],
               [(0, 30), (4, 10), (8, 12), (12, 20)],
               [(0, 20)]])


def test_the_hand_worked_answer():
    units, found = tr.transitions(HAND, 3, 40, UNIT_OF, 3, min_words=2, min_step_works=1)
    assert cells_of(found) == {(0, 1): (2, 2, 1, 0), (1, 0): (1, 0, 1, 0), (1, 1): (1, 1, 1, 1),
                               (1, 2): (1, 1, 1, 1)}
    assert [(c["a"], c["b"]) for c in found] == [(0, 1), (1, 0), (1, 1), (1, 2)]
    assert list(found[0]) == tr.CELL_KEYS and list(units[0]) == tr.UNIT_KEYS
    assert units[1] == dict(passages=4, works=2, starts=1, ends=1, steps_out=3, steps_in=3,
                            successors=3, predecessors=2, best_next=0, best_steps=1)
    assert (units[2]["ends"], units[2]["starts"]) == (2, 1)
    # work 1's first passage has no unit: it starts in unit 1
    assert units[0] == dict(passages=2, works=1, starts=1, ends=0, steps_out=2, steps_in=1,
                            successors=1, predecessors=1, best_next=1, best_steps=2)
    assert (found[0]["steps_out_a"], found[0]["steps_in_b"]) == (2, 3)
    assert sum(u["starts"] for u in units) == sum(u["ends"] for u in units) == 3


def test_within_three_drops_one_step_and_nothing_else():
    free, all_cells = tr.transitions(HAND, 3, 40, UNIT_OF, 3, min_words=2, min_step_works=1)
    units, found = tr.transitions(HAND, 3, 40, UNIT_OF, 3, min_words=2, min_step_works=1, within=3)
    want = cells_of(all_cells)
    want[(0, 1)] = (1, 1, 1, 0)             # fan 11 to fan 20: eight words between
    assert cells_of(found) == want
    for u, v in zip(units, free):
        for k in ("passages", "works", "starts", "ends"):
            assert u[k] == v[k]
    assert (units[0]["steps_out"], units[1]["steps_in"]) == (1, 2)
    # exactly at the bound: fan 1 to fan 5 are three words between, fan 11 to fan 20 eight
    assert cells_of(tr.transitions(HAND, 3, 40, UNIT_OF, 3, 2, 0, 8, 1, 1)[1]) == cells_of(all_cells)
    assert cells_of(tr.transitions(HAND, 3, 40, UNIT_OF, 3, 2, 0, 7, 1, 1)[1]) == want
    assert (0, 1) not in cells_of(tr.transitions(HAND, 3, 40, UNIT_OF, 3, 2, 0, 2, 1, 1)[1])


def test_a_passage_without_a_unit_neither_counts_nor_breaks_a_step():
    # unit 0, then a passage in no unit, then unit 1: one step 0 -> 1 across it
    recs = placed([[(0, 0), (5, 30), (10, 10)]])
    units, found = tr.transitions(recs, 1, 40, UNIT_OF, 3, min_words=2, min_step_works=1)
    assert cells_of(found) == {(0, 1): (1, 1, 1, 0)}
    assert [u["passages"] for u in units] == [1, 1, 0]
    # but the fan words between are those of the two unit-bearing passages: 8
    assert tr.transitions(recs, 1, 40, UNIT_OF, 3, 2, 0, 7, 1, 1)[1] == []
    assert len(tr.transitions(recs, 1, 40, UNIT_OF, 3, 2, 0, 8, 1, 1)[1]) == 1
    # every passage without a unit: zeros and no cells
    units, found = tr.transitions(placed([[(0, 30), (5, 32)]]), 1, 40, UNIT_OF, 3, 2, 0, NONE, 1, 1)
    assert found == [] and all(u == dict(passages=0, works=0, starts=0, ends=0, steps_out=0,
                                         steps_in=0, successors=0, predecessors=0, best_next=NONE,
                                         best_steps=0) for u in units)


def test_the_keep_rule_exactly_at_each_bound():
    # works 0..3 step 0 -> 1 (work 0 twice: 5 steps of 4 works), works 4..8 step 0 -> 2 (5 steps):
    # steps_out(0) = 10, cell (0, 1) is 50 percent of it
    works = [[(0, 0), (5, 10), (10, 0), (15, 10)]] + [[(0, 0), (5, 10)]] * 3 + [[(0, 0), (5, 20)]] * 5
    recs = placed(works)

    def kept(**options):
        return set(cells_of(tr.transitions(recs, 9, 40, UNIT_OF, 3, min_words=2, **options)[1]))
    assert kept(min_step_works=1) == {(0, 1), (0, 2), (1, 0)}
    assert kept(min_steps=5, min_step_works=4) == {(0, 1), (0, 2)}
    assert kept(min_steps=6, min_step_works=1) == set()
    assert kept(min_steps=5, min_step_works=5) == {(0, 2)}
    assert kept(min_step_works=1, min_share=50) == {(0, 1), (0, 2), (1, 0)}
    assert kept(min_step_works=1, min_share=51) == {(1, 0)}           # (1, 0): 1 of 1 step out
    assert kept(min_step_works=1, min_share=100) == {(1, 0)}
    units, found = tr.transitions(recs, 9, 40, UNIT_OF, 3, min_words=2, min_step_works=1,
                                  min_share=51)
    # steps_out and steps_in count every cell, kept or not
    assert (units[0]["steps_out"], units[1]["steps_in"], units[2]["steps_in"]) == (10, 5, 5)
    assert (units[0]["successors"], units[0]["best_next"], units[0]["best_steps"]) == (0, NONE, 0)


def test_best_next_is_the_most_steps_then_the_smaller_unit():
    works = [[(0, 10), (5, 20)], [(0, 10), (5, 0)], [(0, 10), (5, 10)]]
    units, found = tr.transitions(placed(works), 3, 40, UNIT_OF, 3, min_words=2, min_step_works=1)
    assert [(c["a"], c["b"], c["steps"]) for c in found] == [(1, 0, 1), (1, 1, 1), (1, 2, 1)]
    assert (units[1]["best_next"], units[1]["best_steps"], units[1]["successors"]) == (0, 1, 3)
    # one more step to unit 2: the most steps wins over the smaller number
    units, _ = tr.transitions(placed(works + [[(0, 10), (5, 20)]]), 4, 40, UNIT_OF, 3,
                              min_words=2, min_step_works=1)
    assert (units[1]["best_next"], units[1]["best_steps"]) == (2, 2)
    # the cell to unit 0 not kept: the tie goes to the next smaller
    units, _ = tr.transitions(placed(works + [[(0, 10), (5, 20)], [(0, 10), (5, 10)]]), 5, 40,
                              UNIT_OF, 3, min_words=2, min_step_works=2)
    assert (units[1]["best_next"], units[1]["best_steps"], units[1]["successors"]) == (1, 2, 2)


def test_refusals_and_no_records():
    good = placed([[(0, 0)]], words=6)
    unit_of = [0] * 10
    with pytest.raises(ValueError):
        tr.transitions(good + [(1, 0, 0)], 1, 10, unit_of, 1)
    with pytest.raises(ValueError):
        tr.transitions(good[::-1], 1, 10, unit_of, 1)
    with pytest.raises(ValueError):
        tr.transitions(good, 1, 5, unit_of[:5], 1)
    for bad in (dict(min_words=0), dict(min_steps=0), dict(min_step_works=0), dict(min_share=101)):
        with pytest.raises(ValueError):
            tr.transitions(good, 1, 10, unit_of, 1, **bad)
    with pytest.raises(ValueError):
        tr.transitions(good, 1, 10, [1] * 10, 1)
    none = dict(passages=0, works=0, starts=0, ends=0, steps_out=0, steps_in=0, successors=0,
                predecessors=0, best_next=NONE, best_steps=0)
    assert tr.transitions([], 2, 10, unit_of, 1) == ([none], [])
    assert tr.transitions(good, 1, 10, [7] * 3, 0) == ([], [])          # the unit map unread
    assert tr.transitions(good, 1, 10, unit_of, 1, min_words=7) == ([none], [])
    one = dict(none, passages=1, works=1, starts=1, ends=1)
    assert tr.transitions(good, 1, 10, unit_of, 1) == ([one], [])


# ---- the host arithmetic -----------------------------------------------------------------

def test_share_and_lift_in_python_ints():
    assert transitions.share_percent(2, 3) == 66 == tr.share_percent(2, 3)
    assert transitions.lift_permille(5, 20, 10, 5) == 2000 == tr.lift_permille(5, 20, 10, 5)
    assert transitions.lift_permille(1, 3, 3, 1) == 1000
    # numpy's 32-bit values: the products pass 2^64
    big = np.uint32(0xFFFFFFF0)
    want = 0xFFFFFFF0 * 0xFFFFFFF0 * 1000 // (0xFFFFFFF0 * 0xFFFFFFF0)
    assert 0xFFFFFFF0 * 0xFFFFFFF0 * 1000 > 1 << 64
    assert transitions.lift_permille(big, big, big, big) == want == 1000
    assert transitions.share_percent(big, big) == 100
    units = np.zeros(2, dtype=abi.TRANSITION_UNIT_DTYPE)
    units["steps_out"] = [0xFFFFFFF0, 0xFFFFFFF0]
    units["steps_in"] = [0, 0xFFFFFFF0]
    units["best_next"] = [1, NONE]
    cells = np.zeros(1, dtype=abi.TRANSITION_DTYPE)
    cells[0] = (0, 1, 0xFFFFFFF0, 7, 3, 0, 0xFFFFFFF0, 0xFFFFFFF0)
    about = [(0, 9, "HAN", "4", "a b"), (10, 19, "LEIA", "9", "c d")]
    ctab, utab = transitions._rows_of(units, cells, about, ["w.txt"])
    total = 2 * 0xFFFFFFF0
    assert ctab == [[1, 2, 0, 9, "HAN", "4", 10, 19, "LEIA", "9", 0xFFFFFFF0, 7, 3, 100,
                     0xFFFFFFF0 * total * 1000 // (0xFFFFFFF0 * 0xFFFFFFF0), "forward", "w.txt",
                     "a b", "c d"]]
    assert ctab[0][14] == 2000
    assert utab[0][13:15] == [2, 0] and utab[1][13:15] == ["", 0]


def _row(name, fan, fan_word, orig, word, char="HAN", scene="4"):
    return [name, fan, fan_word, 1, orig, word, 2, char, scene, "0.0", 7, "0.0"]


def _match_csv(rows, header=True):
    from tests import passages_restated as pr
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_two_files_of_two_works_going_the_same_way():
    odds, feel = "never tell me the odds".split(), "i have a bad feeling".split()
    rows = []
    for name in ("b.txt", "a.txt"):
        rows += [_row(name, 5 + k, w, 7 + k, w) for k, w in enumerate(odds)]
        rows += [_row(name, 20 + k, w.upper(), 30 + k, w, "LEIA", "9") for k, w in enumerate(feel)]
    cells, units = tr.transitions_csv(_match_csv(rows), min_words=5)
    assert cells.split("\r\n")[1:] == [
        "1,2,7,11,HAN,4,30,34,LEIA,9,2,2,2,100,1000,forward,b.txt,never tell me the odds,"
        "i have a bad feeling", ""]
    assert units.split("\r\n")[1:] == ["1,7,11,HAN,4,2,2,2,0,2,0,1,0,2,2,never tell me the odds",
                                       "2,30,34,LEIA,9,2,2,0,2,0,2,0,1,,0,i have a bad feeling", ""]
    assert tr.transitions_csv(_match_csv(rows, header=False), min_words=5) == (cells, units)
    cells, units = tr.transitions_csv(_match_csv(rows), "character", min_words=5)
    assert cells.split("\r\n")[1:] == ["1,2,7,11,HAN,,30,34,LEIA,,2,2,2,100,1000,forward,b.txt,,", ""]
    free = tr.transitions_csv(_match_csv(rows), min_words=5)
    assert tr.transitions_csv(_match_csv(rows), min_words=5, within=10) == free   # fan 9 to 20
    bound = tr.transitions_csv(_match_csv(rows), min_words=5, within=9)
    assert bound[0].count("\r\n") == 1 and bound[1].split("\r\n")[1].startswith("1,7,11,HAN,4,2,2,2,0,0,0,0,0,,0,")
    assert tr.transitions_csv(_match_csv(rows)) == tuple(
        ",".join(f) + "\r\n" for f in (tr.CELL_FIELDS, tr.UNIT_FIELDS))
    with pytest.raises(ValueError, match="script word 8 has two scenes"):
        tr.transitions_csv(_match_csv(rows + [_row("c.txt", 90, "x", 8, "tell", scene="9")]))


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.build_parser().parse_args(["transitions", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_transitions"
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.within,
            args.min_steps, args.min_step_works, args.min_share, args.device, args.reader) == \
        (None, "region", 6, 0, 1, None, 1, 2, 0, 0, None)
    assert transitions.output_names(args.matches) == (
        "runs/match-6gram-20240101-transitions.csv",
        "runs/match-6gram-20240101-transitions-units.csv")
    assert transitions.output_names("batch", None)[0] == "batch-transitions.csv"
    assert transitions.output_names("m.csv", "out/x")[1] == "out/x-transitions-units.csv"
    args = cli.build_parser().parse_args(
        ["transitions", "m.csv", "-o", "p", "--by", "scene", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--within", "0", "--min-steps", "5", "--min-step-works", "6",
         "--min-share", "75", "--device", "1", "--reader", "python"])
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.within,
            args.min_steps, args.min_step_works, args.min_share, args.device, args.reader) == \
        ("p", "scene", 3, 2, 4, 0, 5, 6, 75, 1, "python")
    assert transitions.CELL_FIELDS == tr.CELL_FIELDS and transitions.UNIT_FIELDS == tr.UNIT_FIELDS
    assert "transitions" in cli.build_parser().format_help()
    assert "transitions" in cli.__doc__
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["transitions", "m.csv", "--by", "word"])


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--min-steps", "0"],
                                 ["--min-step-works", "0"], ["--min-share", "-1"],
                                 ["--min-share", "101"], ["--max-gap", "-1"], ["--within", "-1"],
                                 ["--within", str(NONE)]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["transitions", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py transitions: error: ")


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_transitions", "fs_transitions_rows", "fs_transitions_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.TRANSITIONS_MS_NAMES == ("sequence", "count", "keep", "place", "total")
    assert abi.FS_TRANSITIONS_DENSE == 64


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_transition_unit", "TRANSITION_UNIT_DTYPE", tr.UNIT_KEYS, 40),
    ("fs_transition", "TRANSITION_DTYPE", tr.CELL_KEYS, 32)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for names in re.findall(r"uint32_t\s+([^;]+);", body):
        for n in names.split(","):
            fields.append((n.strip(), at))
            at += 4
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    got = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    units = np.ones(2, dtype=abi.TRANSITION_UNIT_DTYPE)
    found = np.ones(4, dtype=abi.TRANSITION_DTYPE)
    up, fp = units.ctypes.data_as(C.c_void_p), found.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, unit_of=u32, n_units=2, min_words=1, within=NONE, min_steps=1,
             min_step_works=1, min_share=0, out=up, cells=fp, cap=4, n_out=C.byref(got), cols=u32):
        return L.fs_transitions(0, cols, cols, cols, n_rows, 1, n_script, unit_of, n_units,
                                min_words, 0, within, min_steps, min_step_works, min_share, out,
                                cells, cap, n_out)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_steps=0) == abi.FS_E_INVALID
    assert call(min_step_works=0) == abi.FS_E_INVALID
    assert call(min_share=101) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(cells=None) == abi.FS_E_INVALID               # a capacity without a buffer
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["passages"] == 1).all()                     # nothing written by a refusal
    # no records, and no units: units of zeros, no device work
    assert call(n_rows=0, cols=None, unit_of=None, cells=None, cap=0) == abi.FS_OK
    assert got.value == 0
    assert [tuple(u) for u in units.tolist()] == [(0,) * 8 + (NONE, 0)] * 2
    got.value = 7
    assert call(n_units=0, out=None, unit_of=None) == abi.FS_OK and got.value == 0
    assert (found["steps"] == 1).all()
    assert L.fs_transitions_times(None) == abi.FS_E_INVALID
    assert L.fs_transitions_rows(None, None, 0, 0, None, 0, 1, 0, NONE, 1, 1, 0, None, None, 0,
                                 C.byref(got)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        transitions.find_transitions(z, z, z, 1, 5, z, 1)     # a map of 4 entries for 5 words


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, within=NONE, min_steps=1, min_step_works=2, min_share=0, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    units, found = tr.transitions(recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units,
                                  min_words, max_gap, within, min_steps, min_step_works, min_share)
    u = np.array([tuple(r[k] for k in tr.UNIT_KEYS) for r in units],
                 dtype=abi.TRANSITION_UNIT_DTYPE)
    c = np.array([tuple(r[k] for k in tr.CELL_KEYS) for r in found], dtype=abi.TRANSITION_DTYPE)
    return u, c


def oracle_quotes(work, fan_ix, orig_ix, comb, n_works, n_script, min_words=6, max_gap=0,
                  min_works=1, device=0):
    """What the command reads of quotes.find_quotes: the region of each word and the regions'
    first and last words."""
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    unit_of, bounds = cr.regions_of(cr.coverage(recs, n_works, min_words, max_gap), n_script,
                                    min_works)
    words = np.zeros(n_script, dtype=abi.QUOTE_WORD_DTYPE)
    words["region"] = unit_of
    found = np.zeros(len(bounds), dtype=abi.QUOTE_REGION_DTYPE)
    found["first"] = [a for a, _ in bounds]
    found["last"] = [b for _, b in bounds]
    return words, found


def test_the_golden_generator_reproduces_its_committed_files():
    made = mtg.build()
    assert set(made) == {mtg.INPUT} | {n for c in mtg.CASES for n in mtg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name
        assert len(text.encode("utf-8")) < 16 << 10


@pytest.mark.parametrize("case", mtg.CASES, ids=[c[0] for c in mtg.CASES])
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case):
    from fandom_search_amd import companions
    monkeypatch.setattr(transitions, "find_transitions", oracle_find)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    o = mtg.options(case)
    body = transitions.tables(read_matches(os.path.join(GOLDEN, mtg.INPUT)), o["by"],
                              o["min_words"], o["max_gap"], o["min_works"], o["within"],
                              o["min_steps"], o["min_step_works"], o["min_share"])
    for name, head, part in zip(mtg.golden_names(case[0]),
                                (transitions.CELL_FIELDS, transitions.UNIT_FIELDS), body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_input_holds_what_its_generator_says():
    from tests import passages_restated as pr
    rows = pr.read_rows(mtg.input_csv())
    names = [r[0] for r in rows]
    assert len(set(names)) == 12 and 150 <= len(rows) <= 250
    blocks = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
    assert len(blocks) > len(set(blocks))                      # a work comes back
    made = mtg.build()

    def table(case, kind):
        text = made[mtg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    default = table("default", 0)
    assert [(r[0], r[1], r[10], r[15]) for r in default] == [
        ("1", "2", "5", "forward"), ("2", "3", "3", "forward"), ("3", "4", "3", "forward"),
        ("1", "3", "2", "forward"), ("4", "5", "2", "forward")]
    units = table("default", 1)
    assert len(units) == 6 and units[5][5:9] == ["1", "1", "1", "0"]   # f opens on its own line
    assert sum(int(r[7]) for r in units) == sum(int(r[8]) for r in units) == 12
    scene = table("scene", 0)
    assert ("1", "1", "same") in [(r[0], r[1], r[15]) for r in scene]   # scene 4 comes back
    assert ("2", "1", "back") in [(r[0], r[1], r[15]) for r in scene]
    gap = table("gap1_within5_share50", 1)
    # h and i have the fifth line only under --max-gap 1
    assert len(gap) == 5 and (units[4][5], gap[4][5]) == ("2", "4")
    # under --min-works 2 f's own line is no region: f starts in region 1 there
    assert int(gap[0][7]) == int(units[0][7]) + 1
    assert [(r[0], r[1]) for r in table("gap1_within5_share50", 0)] == [
        ("1", "2"), ("2", "3"), ("3", "4"), ("4", "5")]        # g's step is out of reach
