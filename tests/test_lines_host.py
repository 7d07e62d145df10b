"""`ao3.py lines` without a GPU: the line table of the markup against load_markup_script, the
oracle's known answers worked by hand (tests/lines_restated.py), its cross-properties with the
oracles of `pairs` and `companions`, the command's refusals, the C ABI's declarations, and the
committed expected CSVs under the product's table-building code with the oracle standing in for
the device."""

import csv
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, lines, search, synth
from fandom_search_amd.passages import read_matches
from tests import companions_restated as cr
from tests import lines_restated as lr
from tests import passages_restated as pr
from tests.golden import make_lines_golden as mlg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def works_of(spans_of, fan_gap=3):
    """Records (work, fan_ix, orig_ix) of works given as lists of (first script word, words), one
    run behind another in the work with `fan_gap` fan words between them."""
    out = []
    for w, spans in enumerate(spans_of):
        fan = 0
        for orig, words in spans:
            out += [(w, fan + k, orig + k) for k in range(words)]
            fan += words + fan_gap
    return out


# ---- the line table of the markup ----------------------------------------------------------

def markups():
    with open(os.path.join(GOLDEN, "search_golden.json"), encoding="utf-8") as fh:
        cases = json.load(fh)["load_markup_script"]
    out = {name: case["markup"] for name, case in cases.items()}
    out["host_logic"] = ("SCENE_NUMBER<<12A>>\nCHARACTER_NAME<<REY>>\nLINE<<Hello there, General>>\n"
                         "DIRECTION<<She leaves>>\nSCENE_NUMBER<<INT>>\nLINE<<Run>>\n"
                         "SCENE_NUMBER<<40>>\nCHARACTER_NAME<<FINN>>\nLINE<<go  now>>\n")
    out["synthetic"] = synth.script_markup(synth.script_tokens(300), synth.vocab_words())
    out["speeches"] = mlg.SCRIPT
    return out


@pytest.mark.parametrize("name", sorted(markups()))
def test_the_parser_gives_load_markup_script_s_rows_and_lines_that_tile_them(name, tmp_path,
                                                                             capsys):
    text = markups()[name]
    p = tmp_path / "s.txt"
    p.write_text(text, encoding="utf-8")
    rows, line_first = lines.load_markup_lines(str(p))
    assert rows == search.load_markup_script(str(p))
    n = len(rows) - 1
    assert line_first[0] == 0 and line_first[-1] == n
    assert all(a < b for a, b in zip(line_first, line_first[1:])) or n == 0
    if n == 0:
        assert line_first == [0]
    # a line's rows carry one character and one scene
    for a, b in zip(line_first, line_first[1:]):
        assert len({(r[2], r[3]) for r in rows[a + 1:b + 1]}) == 1
    words, restated = lr.markup_lines(text)
    assert restated == line_first
    assert [(w, c, s) for w, _, s, c in rows[1:]] == words


def test_markup_edge_cases(tmp_path):
    p = tmp_path / "s.txt"
    p.write_text("LINE<<before any tag>>\nLINE<<>>\nSCENE_NUMBER<<9>>\nCHARACTER_NAME<<A>>\n"
                 "LINE<<one two>>\nLINE<<  >>\nSCENE_NUMBER<<INT. HALL>>\nLINE<<three>>\n"
                 "SCENE_NUMBER<<40>>\nLINE<<four five six>>\n", encoding="utf-8")
    rows, line_first = lines.load_markup_lines(str(p))
    assert line_first == [0, 3, 5, 6, 9]                  # the two empty LINE tags make no line
    assert rows[1][2:] == [None, None]                    # before any character or scene tag
    assert [rows[a + 1][2] for a in line_first[:-1]] == [None, 9, 2, 3]   # counting from tag 2
    assert [rows[a + 1][3] for a in line_first[:-1]] == [None, "A", "A", "A"]
    assert [r[0] for r in rows[1:]] == "before any tag one two three four five six".split()
    p.write_text("DIRECTION<<nothing spoken>>\n", encoding="utf-8")
    assert lines.load_markup_lines(str(p)) == ([rows[0]], [0])


# ---- oracle known answers, worked by hand ------------------------------------------------

# three lines: words 0..5 (6), 6..9 (4), 10..17 (8); a fourth, 18..19, nobody quotes
FIRST = [0, 6, 10, 18, 20]


def line(**kw):
    base = dict(works=0, whole_works=0, most_works=0, head_works=0, tail_works=0,
                first_work=NONE, covered_sum=0)
    base.update(kw)
    return base


def test_a_line_quoted_whole_its_head_its_tail_and_in_two_pieces():
    recs = works_of([[(10, 8)],                  # whole
                     [(10, 3)],                  # its head
                     [(15, 3)],                  # its tail
                     [(10, 3), (14, 3)],         # two pieces
                     [(12, 3)]])                 # its middle
    found, works, cells = lr.lines(recs, 5, 20, FIRST, min_words=3, most=50)
    assert found == [line(), line(),
                     line(works=5, whole_works=1, most_works=2, head_works=3, tail_works=2,
                          first_work=0, covered_sum=8 + 3 + 3 + 6 + 3),
                     line()]
    assert cells == [dict(line=2, work=0, covered=8, first=10, last=17, runs=1),
                     dict(line=2, work=1, covered=3, first=10, last=12, runs=1),
                     dict(line=2, work=2, covered=3, first=15, last=17, runs=1),
                     dict(line=2, work=3, covered=6, first=10, last=16, runs=2),
                     dict(line=2, work=4, covered=3, first=12, last=14, runs=1)]
    assert works == [dict(work=0, lines=1, whole_lines=1, covered=8, line_words=8, top_line=2,
                          top_covered=8),
                     dict(work=1, lines=1, whole_lines=0, covered=3, line_words=8, top_line=2,
                          top_covered=3),
                     dict(work=2, lines=1, whole_lines=0, covered=3, line_words=8, top_line=2,
                          top_covered=3),
                     dict(work=3, lines=1, whole_lines=0, covered=6, line_words=8, top_line=2,
                          top_covered=6),
                     dict(work=4, lines=1, whole_lines=0, covered=3, line_words=8, top_line=2,
                          top_covered=3)]
    assert list(found[0]) == lr.LINE_KEYS and list(works[0]) == lr.WORK_KEYS
    assert list(cells[0]) == lr.CELL_KEYS
    # --most: 3 of 8 is 37 percent, 6 of 8 is 75; exactly at the bound counts
    assert [lr.lines(recs, 5, 20, FIRST, 3, 0, m)[0][2]["most_works"]
            for m in (1, 37, 38, 75, 76, 100)] == [5, 5, 2, 2, 1, 1]


def test_a_line_twice_in_one_work_counts_once_and_a_work_without_a_passage_for_nothing():
    recs = works_of([[(0, 6), (6, 4), (0, 6)],   # the first line twice
                     [(6, 3)],                   # three stray words at --min-words 4
                     [(0, 6)]])
    found, works, cells = lr.lines(recs, 3, 20, FIRST, min_words=4)
    assert found[0] == line(works=2, whole_works=2, most_works=2, head_works=2, tail_works=2,
                            first_work=0, covered_sum=12)
    assert found[1] == line(works=1, whole_works=1, most_works=1, head_works=1, tail_works=1,
                            first_work=0, covered_sum=4)
    assert [c["work"] for c in cells] == [0, 2, 0]
    # the active works are 0 and 2; on the tie of 6 and 4 ... the larger covered wins
    assert works == [dict(work=0, lines=2, whole_lines=2, covered=10, line_words=10, top_line=0,
                          top_covered=6),
                     dict(work=2, lines=1, whole_lines=1, covered=6, line_words=6, top_line=0,
                          top_covered=6)]


def test_a_passage_across_three_lines_whole_in_the_middle_partial_at_both_ends():
    recs = works_of([[(4, 8)]])                  # words 4..11
    found, works, cells = lr.lines(recs, 1, 20, FIRST)
    assert cells == [dict(line=0, work=0, covered=2, first=4, last=5, runs=1),
                     dict(line=1, work=0, covered=4, first=6, last=9, runs=1),
                     dict(line=2, work=0, covered=2, first=10, last=11, runs=1)]
    assert found[:3] == [line(works=1, tail_works=1, first_work=0, covered_sum=2),
                         line(works=1, whole_works=1, most_works=1, head_works=1, tail_works=1,
                              first_work=0, covered_sum=4),
                         line(works=1, head_works=1, first_work=0, covered_sum=2)]
    assert works == [dict(work=0, lines=3, whole_lines=1, covered=8, line_words=18, top_line=1,
                          top_covered=4)]
    # equal covered in two lines: the earlier line is the top one
    _, works, _ = lr.lines(works_of([[(3, 6)]]), 1, 20, FIRST)
    assert (works[0]["top_line"], works[0]["top_covered"]) == (0, 3)


def test_a_bridged_word_under_max_gap_1_completes_a_line():
    recs = [(0, o, o) for o in range(10, 18) if o != 13]          # 7 records, word 13 left out
    assert lr.lines(recs, 1, 20, FIRST, 6, 0)[1:] == ([], [])     # runs of 3 and 4: no passage
    found, works, cells = lr.lines(recs, 1, 20, FIRST, 6, 1)
    assert cells == [dict(line=2, work=0, covered=8, first=10, last=17, runs=1)]
    assert found[2] == line(works=1, whole_works=1, most_works=1, head_works=1, tail_works=1,
                            first_work=0, covered_sum=8)
    assert works[0]["whole_lines"] == 1


def test_refusals_and_no_records():
    good = works_of([[(0, 6)]])
    with pytest.raises(ValueError):
        lr.lines(good + [(1, 0, 0)], 1, 20, FIRST)
    with pytest.raises(ValueError):
        lr.lines(good[::-1], 1, 20, FIRST)
    with pytest.raises(ValueError):
        lr.lines(good, 1, 5, FIRST)
    for bad in (dict(min_words=0), dict(most=0), dict(most=101)):
        with pytest.raises(ValueError):
            lr.lines(good, 1, 20, FIRST, **bad)
    for table in ([1, 6, 20], [0, 6, 6, 20], [0, 6, 19], [0, 7, 6, 20]):
        with pytest.raises(ValueError):
            lr.lines(good, 1, 20, table)
    assert lr.lines([], 2, 20, FIRST) == ([line()] * 4, [], [])
    assert lr.lines(good, 1, 20, [20]) == ([], [], [])
    assert lr.lines(good, 1, 20, FIRST, min_words=7) == ([line()] * 4, [], [])


# ---- cross-properties --------------------------------------------------------------------

def random_case(rng):
    """Records of a few works over a script of 120 words cut into random lines."""
    n_script = 120
    cuts = sorted(set(rng.choice(np.arange(1, n_script), size=int(rng.integers(1, 30)),
                                 replace=False).tolist()))
    line_first = [0] + cuts + [n_script]
    n_works = int(rng.integers(1, 6))
    recs = []
    for w in range(n_works):
        fan = 0
        for _ in range(int(rng.integers(0, 4))):
            k = int(rng.integers(1, 20))
            o0 = int(rng.integers(0, n_script - k))
            step = rng.choice([1, 2], size=k, p=[0.85, 0.15])
            o = o0 + np.cumsum(step) - step[0]
            o = o[o < n_script]
            recs += [(w, fan + i, int(x)) for i, x in enumerate(o.tolist())]
            fan += len(o) + 5
    return recs, n_works, n_script, line_first


def test_covered_is_the_coverage_and_works_are_those_of_companions_on_300_random_cases():
    rng = np.random.default_rng(11)
    seen_runs2 = seen_partial = 0
    for _ in range(300):
        recs, n_works, n_script, line_first = random_case(rng)
        m, g = int(rng.integers(1, 7)), int(rng.integers(0, 3))
        found, works, cells = lr.lines(recs, n_works, n_script, line_first, m, g)
        cov = cr.coverage(recs, n_works, m, g)
        assert [(v["work"], v["covered"]) for v in works] == \
            [(w, len(c)) for w, c in enumerate(cov) if c]
        line_of = [0] * n_script
        for l in range(len(line_first) - 1):
            line_of[line_first[l]:line_first[l + 1]] = [l] * (line_first[l + 1] - line_first[l])
        units, _ = cr.companions(recs, n_works, n_script, line_of, len(line_first) - 1, m, g)
        assert [v["works"] for v in found] == [u["works"] for u in units]
        assert sum(v["works"] for v in found) == len(cells) == sum(v["lines"] for v in works)
        assert sum(v["covered_sum"] for v in found) == sum(v["covered"] for v in works)
        seen_runs2 += any(c["runs"] >= 2 for c in cells)
        seen_partial += any(c["covered"] < line_first[c["line"] + 1] - line_first[c["line"]]
                            for c in cells)
    assert seen_runs2 > 20 and seen_partial > 100


# ---- the command's refusals, by message --------------------------------------------------

def _files(tmp_path, rows):
    m = tmp_path / "s.txt"
    m.write_text(mlg.SCRIPT, encoding="utf-8")
    buf = io.StringIO(newline="")
    csv.writer(buf).writerows([pr.MATCH_FIELDS] + rows)
    c = tmp_path / "m.csv"
    c.write_text(buf.getvalue(), encoding="utf-8")
    return str(c), str(m)


def _row(name, fan, orig, word):
    return [name, fan, word, 1, orig, word, 2, "HAN", "4", "0.0", 0, "0.0"]


def test_a_file_searched_against_another_script_is_refused_by_name(tmp_path):
    words, _ = lr.markup_lines(mlg.SCRIPT)
    assert len(words) == 68
    good = [_row("a.txt", 5 + k, 4 + k, words[4 + k][0]) for k in range(7)]
    src, markup = _files(tmp_path, good + [_row("a.txt", 40, 68, "beyond")])
    with pytest.raises(SystemExit) as e:
        cli.main(["lines", src, markup, "--reader", "python"])
    assert str(e.value.code) == (
        "ao3.py lines: error: ORIGINAL_SCRIPT_WORD_INDEX 68 in a script markup of 68 words (the "
        "records need at least 69): was the file searched against another script?")
    with pytest.raises(ValueError, match="INDEX 68 in a script markup of 68 words"):
        lr.lines_csv(open(src, newline="", encoding="utf-8").read(), mlg.SCRIPT)
    # a word that differs: the smallest script word index, its first record that differs
    bad = good + [_row("b.txt", 1, 9, "odd"), _row("b.txt", 2, 6, "a"), _row("b.txt", 3, 6, "the"),
                  _row("b.txt", 4, 6, "an")]
    src, markup = _files(tmp_path, bad)
    with pytest.raises(SystemExit) as e:
        cli.main(["lines", src, markup, "--reader", "python"])
    assert str(e.value.code) == (
        "ao3.py lines: error: script word 6 is 'the' in the records and 'a' in the script "
        "markup: was the file searched against another script?")
    with pytest.raises(ValueError, match="script word 6 is 'the' in the records and 'a'"):
        lr.lines_csv(open(src, newline="", encoding="utf-8").read(), mlg.SCRIPT)


@pytest.mark.parametrize("bad,message", [
    (["--most", "0"], "--most must be from 1 to 100"),
    (["--most", "101"], "--most must be from 1 to 100"),
    (["--min-words", "0"], "--min-words and --min-works must be at least 1, --max-gap at least 0"),
    (["--min-works", "0"], "--min-words and --min-works must be at least 1, --max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words and --min-works must be at least 1, --max-gap at least 0")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["lines", str(tmp_path / "none.csv"), str(tmp_path / "none.txt")] + bad)
    assert str(e.value.code) == "ao3.py lines: error: " + message


def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["lines", "runs/match-6gram-20240101.csv", "script.txt"])
    assert args.func.__name__ == "_lines"
    assert (args.script, args.output, args.min_words, args.max_gap, args.min_works, args.most,
            args.device, args.reader) == ("script.txt", None, 6, 0, 1, 50, 0, None)
    assert lines.output_names(args.matches) == (
        "runs/match-6gram-20240101-lines.csv", "runs/match-6gram-20240101-lines-works.csv",
        "runs/match-6gram-20240101-lines-cells.csv")
    assert lines.output_names("m.csv", "out/x")[2] == "out/x-lines-cells.csv"
    args = cli.ao3_parser().parse_args(
        ["lines", "m.csv", "s.txt", "-o", "p", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--most", "75", "--device", "1", "--reader", "python"])
    assert (args.output, args.min_words, args.max_gap, args.min_works, args.most, args.device,
            args.reader) == ("p", 3, 2, 4, 75, 1, "python")
    assert (lines.LINE_FIELDS, lines.WORK_FIELDS, lines.CELL_FIELDS) == \
        (lr.LINE_FIELDS, lr.WORK_FIELDS, lr.CELL_FIELDS)
    assert "lines" in cli.ao3_parser().format_help()
    # the parsers whose surfaces are pinned do not know the command
    with pytest.raises(SystemExit):
        cli.full_parser().parse_args(["lines", "m.csv", "s.txt"])


# ---- the C ABI ---------------------------------------------------------------------------

def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_lines", "fs_lines_rows", "fs_lines_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.LINES_MS_NAMES == ("tables", "walk", "total")
    assert re.search(r"#define FS_LINES_MAX_BYTES \(1u << 30\)", text)
    assert abi.FS_LINES_MAX_BYTES == 1 << 30


@pytest.mark.parametrize("struct,dtype,keys", [
    ("fs_line", "LINE_DTYPE", lr.LINE_KEYS),
    ("fs_line_work", "LINE_WORK_DTYPE", lr.WORK_KEYS + ["reserved"]),
    ("fs_line_cell", "LINE_CELL_DTYPE", lr.CELL_KEYS + ["reserved", "reserved2"])])
def test_dtypes_match_the_header(struct, dtype, keys):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for bits, names in re.findall(r"uint(32|64)_t\s+([^;]+);", body):
        for n in names.split(","):
            assert at % (int(bits) // 8) == 0
            fields.append((n.strip(), at))
            at += int(bits) // 8
    dt = getattr(abi, dtype)
    assert dt.itemsize == at == 32                             # a power of two
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n_active, n_cells = C.c_uint64(7), C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    table = np.array([0, 2, 4], dtype=np.uint32)
    u32, tp = abi.ptr(z, C.c_uint32), abi.ptr(table, C.c_uint32)
    found = np.ones(2, dtype=abi.LINE_DTYPE)
    works = np.ones(2, dtype=abi.LINE_WORK_DTYPE)
    cells = np.ones(2, dtype=abi.LINE_CELL_DTYPE)
    lp, wp, cp = (x.ctypes.data_as(C.c_void_p) for x in (found, works, cells))

    def call(n_rows=1, n_script=4, line_first=tp, n_lines=2, min_words=1, most=50, out=lp,
             w_out=wp, w_cap=2, na=C.byref(n_active), c_out=cp, c_cap=2, nc=C.byref(n_cells),
             cols=u32):
        return L.fs_lines(0, cols, cols, cols, n_rows, 1, n_script, line_first, n_lines,
                          min_words, 0, most, out, w_out, w_cap, na, c_out, c_cap, nc)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(most=0) == abi.FS_E_INVALID
    assert call(most=101) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(w_out=None) == abi.FS_E_INVALID                # a capacity without a buffer
    assert call(c_out=None) == abi.FS_E_INVALID
    assert call(na=None) == abi.FS_E_INVALID
    assert call(nc=None) == abi.FS_E_INVALID
    assert call(line_first=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (found["works"] == 1).all()                         # nothing written by a refusal
    # no records, and no lines: lines nobody quotes, no device work
    assert call(n_rows=0, cols=None, line_first=None, w_out=None, w_cap=0, c_out=None,
                c_cap=0) == abi.FS_OK
    assert (n_active.value, n_cells.value) == (0, 0)
    assert [tuple(v) for v in found.tolist()] == [(0, 0, 0, 0, 0, NONE, 0)] * 2
    n_active.value = n_cells.value = 7
    assert call(n_lines=0, out=None, line_first=None) == abi.FS_OK
    assert (n_active.value, n_cells.value) == (0, 0)
    assert (works["lines"] == 1).all() and (cells["covered"] == 1).all()
    assert L.fs_lines_times(None) == abi.FS_E_INVALID
    assert L.fs_lines_rows(None, None, 0, 0, None, 0, 1, 0, 50, None, None, 0,
                           C.byref(n_active), None, 0, C.byref(n_cells)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        lines.find_lines(z, z[:3], z, 1, 4, table)             # columns of different lengths


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, line_first, min_words=6, max_gap=0,
                most=50, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    found, works, cells = lr.lines(recs, n_works, n_script, list(line_first), min_words, max_gap,
                                   most)
    return (np.array([tuple(r[k] for k in lr.LINE_KEYS) for r in found], dtype=abi.LINE_DTYPE),
            np.array([tuple(r[k] for k in lr.WORK_KEYS) + (0,) for r in works],
                     dtype=abi.LINE_WORK_DTYPE),
            np.array([tuple(r[k] for k in lr.CELL_KEYS) + (0, 0) for r in cells],
                     dtype=abi.LINE_CELL_DTYPE))


def test_the_golden_generator_reproduces_its_committed_files():
    made = mlg.build()
    assert set(made) == {mlg.MARKUP, mlg.INPUT} | {n for c in mlg.CASES
                                                   for n in mlg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,min_words,max_gap,min_works,most", mlg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, min_words, max_gap,
                                                      min_works, most):
    monkeypatch.setattr(lines, "find_lines", oracle_find)
    markup = lines.load_markup_lines(os.path.join(GOLDEN, mlg.MARKUP))
    body = lines.tables(read_matches(os.path.join(GOLDEN, mlg.INPUT)), markup, min_words,
                        max_gap, min_works, most)
    heads = (lines.LINE_FIELDS, lines.WORK_FIELDS, lines.CELL_FIELDS)
    for name, head, part in zip(mlg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_files_hold_what_their_generator_says():
    made = mlg.build()
    words, line_first = lr.markup_lines(mlg.SCRIPT)
    assert len(line_first) - 1 == 12
    assert len({c for _, c, _ in words}) == 4 and {s for _, _, s in words} == {None, 4, 7, 3}

    def table(case, kind):
        text = made[mlg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    default = table("default", 0)
    assert [r[0] for r in default] == ["12", "2", "7", "10", "11", "3", "6", "8"]
    # "i have a bad feeling about this": four works, two whole, b its head, c its tail
    assert default[1][6:13] == ["4", "2", "4", "3", "3", "92", "50"]
    cells = table("default", 2)
    assert [r[7] for r in cells if r[1] == "e.txt"] == ["2"]   # two pieces
    assert [(r[0], r[8]) for r in cells if r[1] == "d.txt"] == [("6", "0"), ("7", "1"), ("8", "0")]
    assert sum(1 for r in cells if (r[0], r[1]) == ("12", "dir/c.txt")) == 1   # twice: one cell
    assert not [r for r in cells if r[1] in ("f.txt", "h.txt")]
    gap1 = table("gap1_most80", 2)
    assert [r[2:9] for r in gap1 if r[1] == "f.txt"] == [["7", "7", "100", "48", "54", "1", "1"]]
    assert [r[8] for r in table("gap1_most80", 0) if r[0] == "8"] == ["0"]     # 60 < 80
    assert [r[0] for r in table("minworks2", 0)] == ["12", "2"]
