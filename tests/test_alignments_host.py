"""`ao3.py alignments` without a GPU: the restated rule (tests/alignments_restated.py) on
hand-worked records, its agreement with the passages of `--max-gap 0` at reach 0, the committed
expected files, the command line's argument checks and the ABI's Python side."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, alignments, cli
from fandom_search_amd.passages import read_matches
from tests import alignments_restated as ar
from tests import passages_restated as pr
from tests.golden import make_alignments_golden as mag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MESSAGE = ("--min-words and --match must be at least 1, --reach from 0 to 63, --gap from 0 to "
           "16, --match at most 16")


def recs(pairs, work=0, comb=0.0):
    return [(work, f, o, comb) for f, o in pairs]


def diagonal(fan, orig, count):
    return [(fan + k, orig + k) for k in range(count)]


# ---- the rule, by hand ---------------------------------------------------------------------

EIGHT = diagonal(10, 100, 3) + [(13, 700)] + diagonal(14, 103, 3) + diagonal(17, 107, 2)


def test_the_eight_word_example_field_by_field():
    records = recs(EIGHT)
    best, prev = ar.chain(records)
    assert best == [2, 4, 6, 2, 7, 9, 11, 12, 14]
    assert prev == [None, 0, 1, None, 2, 4, 5, 6, 7]
    found, path = ar.alignments(records)
    assert found == [dict(first=0, last=8, n_words=8, n_exact=8, score=14, fan_skipped=1,
                          orig_skipped=1, pieces=3, tree_records=8, reserved=0, path_at=0)]
    assert path == [0, 1, 2, 4, 5, 6, 7, 8]
    # `passages` finds nothing in it, bridging or not
    five = [r + (0.0,) for r in records]
    assert pr.passages(five, 6, 0) == [] and pr.passages(five, 6, 1) == []
    # the stray record is a tree of one record, listed only when one word is enough
    found, path = ar.alignments(records, min_words=1)
    assert [(a['first'], a['n_words'], a['tree_records'], a['path_at']) for a in found] == [
        (0, 8, 8, 0), (3, 1, 1, 8)]
    assert path == [0, 1, 2, 4, 5, 6, 7, 8, 3]


def test_a_tie_between_two_predecessors_goes_to_the_nearer_one():
    # record 1 steps back in the script, so it is a root like record 0; record 2 is two fan and
    # two script words past record 0, one fan and three script words past record 1: cost 2 each
    records = recs([(1, 10), (2, 9), (3, 12)])
    assert ar.chain(records, match=4, gap=1) == ([4, 4, 6], [None, None, 1])
    assert ar.chain(records, match=2, gap=0) == ([2, 2, 4], [None, None, 1])
    assert ar.chain(records, match=2, gap=1) == ([2, 2, 2], [None, None, None])   # 2 - 2 is not above 0
    # a better value beats a nearer record
    records = recs([(1, 10), (2, 9), (3, 11)])                # cost 1 from record 0, 1 from 1
    assert ar.chain(records, match=4, gap=1)[1] == [None, None, 1]
    records = recs([(1, 10), (2, 7), (3, 11)])                # cost 1 from record 0, 3 from 1
    assert ar.chain(records, match=4, gap=1) == ([4, 4, 7], [None, None, 0])


def test_equal_values_take_the_largest_j():
    # records 1 and 2 stand at one fan index with the same best and the same cost to record 3
    records = recs([(1, 10), (2, 11), (2, 11), (3, 12)])
    best, prev = ar.chain(records)
    assert best == [2, 4, 4, 6] and prev == [None, 0, 0, 2]
    found, path = ar.alignments(records, min_words=1)
    assert len(found) == 1 and path == [0, 2, 3] and found[0]['tree_records'] == 4


def test_a_peak_tie_goes_to_the_earlier_record():
    # the trunk 0, 1 and two leaves of equal best at one fan index
    records = recs([(1, 10), (2, 11), (3, 12), (3, 13)], comb=1.0)
    best, prev = ar.chain(records, gap=0)
    assert best == [2, 4, 6, 6] and prev == [None, 0, 1, 1]
    found, path = ar.alignments(records, min_words=1, gap=0)
    assert [(a['last'], a['n_words'], a['tree_records'], a['n_exact']) for a in found] == [
        (2, 3, 4, 0)]
    assert path == [0, 1, 2]


def test_an_interior_peak_the_path_stops_short_of_a_costly_last_link():
    records = recs(diagonal(1, 100, 6) + [(10, 108)])
    best, prev = ar.chain(records)
    assert best[-2:] == [12, 9] and prev[-1] == 5
    found, path = ar.alignments(records)
    assert len(found) == 1 and path == [0, 1, 2, 3, 4, 5]
    a = found[0]
    assert (a['last'], a['n_words'], a['score'], a['tree_records'], a['pieces']) == (5, 6, 12, 7, 1)


def test_a_trunk_with_two_branches_is_one_alignment():
    trunk = diagonal(1, 100, 4)
    records = recs(trunk + [(5, 104), (5, 110), (6, 105), (6, 111), (7, 106)])
    # 110 lies out of the trunk's reach: a tree of its own with 111
    found, path = ar.alignments(records, min_words=1)
    assert [(a['first'], a['last'], a['n_words'], a['tree_records']) for a in found] == [
        (0, 8, 7, 7), (5, 7, 2, 2)]
    records = recs(trunk + [(5, 104), (5, 106), (6, 105), (6, 107), (7, 106)])
    found, path = ar.alignments(records, min_words=1)
    assert len(found) == 1
    a = found[0]
    assert (a['n_words'], a['tree_records'], a['score']) == (7, 9, 14)
    assert path == [0, 1, 2, 3, 4, 6, 8]                      # 5 and 7 are side records


def test_the_script_side_must_advance_and_one_fan_index_never_links():
    assert ar.chain(recs([(1, 10), (2, 10)]))[1] == [None, None]          # do == 0
    assert ar.chain(recs([(1, 10), (2, 9)]))[1] == [None, None]           # do < 0
    assert ar.chain(recs([(1, 10), (1, 11)]))[1] == [None, None]          # df == 0
    assert ar.chain(recs([(1, 10), (2, 11)]))[1] == [None, 0]
    assert ar.chain([(0, 1, 10, 0.0), (1, 2, 11, 0.0)])[1] == [None, None]   # two works
    # the far edge of reach on either side
    for reach in (0, 3, 63):
        for step, linked in ((reach + 1, True), (reach + 2, False)):
            for pair in ((1 + step, 11), (2, 10 + step)):
                got = ar.chain(recs([(1, 10), pair]), reach=reach, match=16, gap=0)[1][1]
                assert (got == 0) == linked, (reach, pair)


def test_nan_is_never_exact_and_refusals():
    records = [(0, 1, 10, float('nan')), (0, 2, 11, 0.0), (0, 3, 12, -1.0), (0, 4, 13, 0.5)]
    found, _ = ar.alignments(records, min_words=1)
    assert found[0]['n_exact'] == 2 and found[0]['n_words'] == 4
    assert ar.alignments([], 6) == ([], [])
    for bad in (dict(min_words=0), dict(match=0), dict(reach=64), dict(match=17), dict(gap=17)):
        with pytest.raises(ValueError):
            ar.alignments(records, **bad)
    with pytest.raises(ValueError):
        ar.alignments(records[::-1])
    with pytest.raises(NotImplementedError):
        ar.check(1 << 32, 6, 4, 2, 1)
    with pytest.raises(NotImplementedError):
        ar.check(1 << 28, 6, 4, 16, 1)
    ar.check((1 << 28) - 1, 6, 4, 16, 1)


# ---- reach 0 is `passages --max-gap 0` --------------------------------------------------

def random_records(rng):
    """Under 400 records of a few works, fan indices strictly rising inside a work: runs that
    step together, broken by jumps on either side."""
    out = []
    for work in range(int(rng.integers(1, 6))):
        fan, orig = int(rng.integers(0, 5)), int(rng.integers(0, 50))
        for _ in range(int(rng.integers(0, 75))):
            out.append((work, fan, orig, float(rng.choice([0.0, 0.25, float('nan')]))))
            kind = rng.random()
            fan += 1 if kind < 0.8 else int(rng.integers(1, 4))
            orig += 1 if kind < 0.85 else int(rng.integers(-3, 4))
            orig = max(orig, 0)
    return out


def test_at_reach_0_the_alignments_are_the_passages_of_max_gap_0():
    rng = np.random.default_rng(11)
    kept = 0
    for _ in range(300):
        records = random_records(rng)
        assert len(records) < 400
        for min_words in (1, 3, 6):
            found, path = ar.alignments(records, min_words, reach=0,
                                        match=int(rng.integers(1, 17)), gap=int(rng.integers(0, 17)))
            want = pr.passages([r[:3] + (0.0, r[3]) for r in records], min_words, 0)
            assert [(a['first'], a['n_words'], a['n_exact']) for a in found] == [
                (p['first'], p['n_words'], p['n_exact']) for p in want]
            assert all(a['pieces'] == 1 and a['tree_records'] == a['n_words']
                       and a['last'] == a['first'] + a['n_words'] - 1 for a in found)
            assert path == [i for p in want for i in range(p['first'], p['first'] + p['n_words'])]
            kept += len(found)
    assert kept > 1000


# ---- the two files -------------------------------------------------------------------------

def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(ar.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_two_files_of_the_eight_word_example():
    words = "may the force be with you now and always".split()
    rows = []
    for k, (f, o) in enumerate(EIGHT):
        stray = o == 700
        rows.append(["w.txt", f, "always" if stray else words[o - 100], 1, o,
                     "ever" if stray else words[o - 100], 2, "OBI", "7",
                     "" if k == 1 else 0.5 if stray else 0.0, 0,
                     "" if k == 1 else 0.5 if k == 4 else 0.0])
    aligned, works = ar.alignments_csv(_match_csv(rows))
    assert ar.alignments_csv(_match_csv(rows, header=False)) == (aligned, works)
    body = list(csv.reader(io.StringIO(aligned, newline="")))
    assert body[0] == ar.ALIGNMENT_FIELDS and len(body) == 2
    assert body[1] == ["w.txt", "10", "18", "100", "108", "8", "6", "14", "1", "1", "3", "0", "OBI",
                       "7", "nan", "0.5", "may the force [+1] be with you and always",
                       "may the force be with you [+1] and always"]
    assert list(csv.reader(io.StringIO(works, newline=""))) == [
        ar.WORK_FIELDS, ["w.txt", "1", "8", "8", "1", "1", "0", "8"]]
    assert ar.alignments_csv(_match_csv(rows), reach=0) == (
        _match_csv([ar.ALIGNMENT_FIELDS], header=False), _match_csv([ar.WORK_FIELDS], header=False))


def test_the_golden_generator_reproduces_its_committed_files():
    made = mag.build()
    assert set(made) == {mag.INPUT, mag.CLI} | {n for c in mag.CASES for n in mag.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


def test_the_committed_files_are_the_restatement_of_the_committed_input():
    with open(os.path.join(GOLDEN, mag.INPUT), encoding="utf-8", newline="") as fh:
        text = fh.read()
    for case, min_words, reach, match, gap in mag.CASES:
        for name, part in zip(mag.golden_names(case),
                              ar.alignments_csv(text, min_words, reach, match, gap)):
            with open(os.path.join(GOLDEN, name), "rb") as fh:
                assert fh.read() == part.encode("utf-8"), name


def test_the_golden_input_holds_what_its_generator_says():
    rows = ar.read_rows(mag.input_csv())
    names = [r[0] for r in rows]
    assert len(set(names)) == 12 and 100 <= len(rows) <= 200
    blocks = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
    assert len(blocks) > len(set(blocks))                      # a work comes back
    fans = {r[2] for r in rows}
    assert any("," in f for f in fans) and any('"' in f for f in fans)
    assert any(not f.isascii() for f in fans)
    assert any(a[:2] == b[:2] for a, b in zip(rows, rows[1:]))  # two records at one fan index
    made = mag.build()

    def table(case, kind):
        return [r for r in csv.reader(io.StringIO(made[mag.golden_names(case)[kind]], newline=""))][1:]
    default = table("default", 0)
    by_work = {}
    for r in default:
        by_work.setdefault(r[0], []).append(r)
    assert set(by_work) == set(names) - {"f.txt", "k.txt"}     # strays only; too short
    b = by_work["b.txt"][0]
    assert b[5:12] == ["8", "8", "14", "1", "1", "3", "0"]     # the inserted and the dropped word
    assert b[-2:] == ["i have a [+1] very bad feeling all this",
                      "i have a very bad feeling [+1] all this"]
    assert len(by_work["d.txt"]) == 2                          # swapped halves: two alignments
    assert [r[3] for r in by_work["d.txt"]] == ["227", "220"]
    assert by_work["dir/c.txt"][0][6] == "5"                   # a substituted word with a record
    assert by_work["m.txt"][0][5:12] == ["6", "6", "12", "0", "0", "1", "1"]   # an interior peak
    assert by_work["e.txt"][1][11] == "1"                      # a side record
    works = {r[0]: r for r in table("default", 1)}
    assert works["b.txt"][1:] == ["1", "8", "8", "1", "1", "0", "8"]
    assert works["a.txt"][-1] == "0" and works["i.txt"][-1] == "10"
    assert "b.txt" not in {r[0] for r in table("reach0", 0)}
    assert "i.txt" not in {r[0] for r in table("reach1_gap2", 0)}
    assert "b.txt" in {r[0] for r in table("reach1_gap2", 0)}


# ---- product side that needs no GPU --------------------------------------------------------

def as_arrays(found, path):
    a = np.array([tuple(r[k] for k in ar.KEYS) for r in found], dtype=abi.ALIGNMENT_DTYPE)
    return a, np.asarray(path, dtype=np.uint32)


def oracle_find(work, fan_ix, orig_ix, comb, min_words=6, reach=4, match=2, gap=1, device=0):
    records = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix, comb))))
    return as_arrays(*ar.alignments(records, min_words, reach, match, gap))


def oracle_passages(work, fan_ix, orig_ix, dist, comb, min_words=6, max_gap=0, device=0):
    records = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix, dist, comb))))
    found = pr.passages(records, min_words, max_gap)
    return np.array([tuple(p[k] for k in abi.PASSAGE_DTYPE.names) for p in found],
                    dtype=abi.PASSAGE_DTYPE)


@pytest.mark.parametrize("case,min_words,reach,match,gap", mag.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, min_words, reach, match,
                                                      gap):
    monkeypatch.setattr(alignments, "find_alignments", oracle_find)
    monkeypatch.setattr(alignments, "find_passages", oracle_passages)
    body = alignments.tables(read_matches(os.path.join(GOLDEN, mag.INPUT)), min_words, reach, match,
                             gap)
    for name, head, part in zip(mag.golden_names(case),
                                (alignments.ALIGNMENT_FIELDS, alignments.WORK_FIELDS), body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_command_line_s_surface():
    """cli.build_parser() keeps the surface tests/golden/cli_surface.json pins; cli.full_parser(),
    which `ao3.py` runs, has the same commands and `alignments` behind them, pinned by
    tests/golden/alignments_cli.json."""
    import json
    from tests.golden.make_cli_surface import surface
    with open(os.path.join(GOLDEN, "cli_surface.json"), encoding="utf-8") as fh:
        pinned = json.load(fh)
    with open(os.path.join(GOLDEN, mag.CLI), encoding="utf-8") as fh:
        mine = json.load(fh)
    assert json.loads(json.dumps(surface(cli.build_parser()))) == pinned
    assert json.loads(json.dumps(surface(cli.full_parser()))) == pinned + [mine]
    assert mine[0] == "alignments"
    assert [a["dest"] for a in mine[2]] == ["help", "matches", "output", "min_words", "reach",
                                            "match", "gap", "device", "reader"]
    assert "alignments" not in [s[0] for s in pinned]


def test_parser_defaults_and_output_names():
    args = cli.full_parser().parse_args(["alignments", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_alignments"
    assert (args.output, args.min_words, args.reach, args.match, args.gap, args.device,
            args.reader) == (None, 6, 4, 2, 1, 0, None)
    assert not hasattr(args, "max_gap")
    assert alignments.output_names(args.matches) == (
        "runs/match-6gram-20240101-alignments.csv",
        "runs/match-6gram-20240101-alignments-works.csv")
    assert alignments.output_names("m.csv", "out/x")[1] == "out/x-alignments-works.csv"
    args = cli.full_parser().parse_args(
        ["alignments", "m.csv", "-o", "p", "--min-words", "3", "--reach", "63", "--match", "16",
         "--gap", "0", "--device", "1", "--reader", "python"])
    assert (args.output, args.min_words, args.reach, args.match, args.gap, args.device,
            args.reader) == ("p", 3, 63, 16, 0, 1, "python")
    assert alignments.ALIGNMENT_FIELDS == ar.ALIGNMENT_FIELDS
    assert alignments.WORK_FIELDS == ar.WORK_FIELDS
    assert "alignments" in cli.full_parser().format_help()


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--match", "0"], ["--match", "17"],
                                 ["--reach", "-1"], ["--reach", "64"], ["--gap", "-1"],
                                 ["--gap", "17"], ["--min-words", "-3", "--gap", "99"]])
def test_every_argument_check_exits_before_the_library_loads(bad, tmp_path, monkeypatch):
    def load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", load)
    monkeypatch.setattr(alignments, "process", load)
    with pytest.raises(SystemExit) as e:
        cli.main(["alignments", str(tmp_path / "none.csv")] + bad)
    assert e.value.code == "ao3.py alignments: error: " + MESSAGE


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_alignments", "fs_alignments_rows", "fs_alignments_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "alignments" in _lib.TIMED
    assert len(abi.ALIGNMENTS_MS_NAMES) == 6 and abi.ALIGNMENTS_MS_NAMES[-1] == "total"
    for name in ("FS_ALIGNMENTS_SMALL", "FS_ALIGNMENTS_RING"):
        assert name in text
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_the_dtype_matches_the_header_56_bytes():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct fs_alignment \{(.*?)\} fs_alignment;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for kind, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body):
        for n in names.split(","):
            fields.append((n.strip(), at))
            at += 8 if kind == "uint64_t" else 4
    dt = abi.ALIGNMENT_DTYPE
    assert dt.itemsize == 56 == at
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert dt.fields["path_at"][1] == 48 and dt.fields["n_words"][1] == 16
    assert list(dt.names) == ar.KEYS
    assert "56 bytes" in re.search(r"\} fs_alignment;[^\n]*", text).group(0)


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    got, got_path = C.c_uint64(7), C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    d = np.zeros(4, dtype=np.float64)
    u32, f64 = abi.ptr(z, C.c_uint32), abi.ptr(d, C.c_double)
    found = np.ones(4, dtype=abi.ALIGNMENT_DTYPE)
    path = np.ones(4, dtype=np.uint32)
    fp, pp = found.ctypes.data_as(C.c_void_p), path.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, min_words=1, reach=4, match=2, gap=1, out=fp, cap=4, n_out=C.byref(got),
             to=pp, path_cap=4, n_path=C.byref(got_path), cols=u32, comb=f64):
        return L.fs_alignments(0, cols, cols, cols, comb, n_rows, min_words, reach, match, gap,
                               out, cap, n_out, to, path_cap, n_path)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_rows=1 << 28, match=16) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(match=0) == abi.FS_E_INVALID
    assert call(reach=64) == abi.FS_E_INVALID
    assert call(match=17) == abi.FS_E_INVALID
    assert call(gap=17) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID                 # a capacity without a buffer
    assert call(to=None) == abi.FS_E_INVALID
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(n_path=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert call(comb=None) == abi.FS_E_INVALID
    # no records: nothing found, no device work
    assert call(n_rows=0, cols=None, comb=None, out=None, cap=0, to=None, path_cap=0) == abi.FS_OK
    assert got.value == 0 and got_path.value == 0
    assert (found["n_words"] == 1).all() and (path == 1).all()
    ms = (C.c_double * 6)(*[9.0] * 6)
    assert L.fs_alignments_times(ms) == abi.FS_OK and list(ms) == [0.0] * 6
    assert L.fs_alignments_times(None) == abi.FS_E_INVALID
    assert L.fs_alignments_rows(None, None, 0, 1, 4, 2, 1, None, 0, C.byref(got), None, 0,
                                C.byref(got_path)) == abi.FS_E_INVALID
