"""`bundles` without a GPU: the restated contract (tests/bundles_restated.py) against a brute
force that takes every subset directly, hand-made answers, the LIFT arithmetic, the command
line, the ABI, and the committed expected outputs."""

import csv
import ctypes as C
import io
import itertools
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, bundles, cli
from fandom_search_amd.passages import read_matches
from tests import bundles_restated as br
from tests.golden import make_bundles_golden as mbg
from tests.test_companions_host import oracle_quotes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = br.NONE


# ---- the restatement against a brute force ----------------------------------------------

def brute(members, min_all, max_size):
    """Every subset of 2 .. max_size + 1 units taken directly, no levels: {set: works} of the
    frequent ones, and from those the records of the listed sizes."""
    n_units = len(members)
    freq = {}
    for k in range(2, max_size + 2):
        for s in itertools.combinations(range(n_units), k):
            works = set.intersection(*(members[u] for u in s))
            if len(works) >= min_all:
                freq[s] = works
    sets = []
    for s in sorted((s for s in freq if len(s) <= max_size), key=lambda s: (len(s), s)):
        bigger = [t for t in freq if len(t) == len(s) + 1 and set(s) < set(t)]
        sets.append(dict(units=list(s) + [NONE] * (8 - len(s)), size=len(s),
                         works=len(freq[s]), first_work=min(freq[s]), extensions=len(bigger),
                         closed=int(all(len(freq[t]) != len(freq[s]) for t in bigger))))
    return freq, sets


@pytest.mark.parametrize("seed", range(12))
def test_the_level_wise_restatement_equals_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    n_units, n_works = int(rng.integers(2, 13)), int(rng.integers(1, 41))
    density = (0.2, 0.5, 0.8)[seed % 3]
    members = [set(np.nonzero(rng.random(n_works) < density)[0].tolist())
               for _ in range(n_units)]
    for min_all, max_size in ((1, 2), (2, 4), (3, 8), (1, 8), (5, 3)):
        freq, want = brute(members, min_all, max_size)
        units, levels, sets = br.mine(members, min_all, max_size)
        assert sets == want
        assert [v['size'] for v in levels] == list(range(2, max_size + 2))
        for v in levels:
            k = v['size']
            assert v['frequent'] == sum(1 for s in freq if len(s) == k)
            of_size = [s for s in want if s['size'] == k]
            if k <= max_size:
                assert v['closed'] == sum(s['closed'] for s in of_size)
                assert v['maximal'] == sum(s['extensions'] == 0 for s in of_size)
            else:
                assert v['closed'] == v['maximal'] == NONE
            assert v['candidates'] >= v['frequent']
        single = sum(1 for m in members if len(m) >= min_all)
        assert levels[0]['candidates'] == single * (single - 1) // 2
        for u, v in enumerate(units):
            mine = [s for s in want if u in s['units'][:s['size']]]
            assert v == dict(works=len(members[u]), sets=len(mine),
                             largest=max([s['size'] for s in mine], default=0))


# ---- hand-made answers ------------------------------------------------------------------

def test_a_clique_of_four_units_only_the_set_of_four_is_closed():
    members = [set(range(5)) for _ in range(4)] + [set()]
    units, levels, sets = br.mine(members, 5, 4)
    assert [(s['size'], s['closed'], s['extensions']) for s in sets] == \
        [(2, 0, 2)] * 6 + [(3, 0, 1)] * 4 + [(4, 1, 0)]
    assert all(s['works'] == 5 and s['first_work'] == 0 for s in sets)
    assert sets[-1]['units'] == [0, 1, 2, 3] + [NONE] * 4
    assert [(v['candidates'], v['frequent'], v['closed'], v['maximal']) for v in levels] == \
        [(6, 6, 0, 0), (4, 4, 0, 0), (1, 1, 1, 1), (0, 0, NONE, NONE)]
    assert units[:4] == [dict(works=5, sets=7, largest=4)] * 4
    assert units[4] == dict(works=0, sets=0, largest=0)
    # --max-size 3: the set of four is mined, marks the sets of three and is not listed
    units, levels, sets = br.mine(members, 5, 3)
    assert len(sets) == 10 and not any(s['closed'] for s in sets)
    assert levels[2] == dict(size=4, candidates=1, frequent=1, closed=NONE, maximal=NONE)
    assert units[0] == dict(works=5, sets=6, largest=3)


def test_a_unit_below_min_all_and_min_all_of_one():
    members = [{0, 1, 2, 3, 4}, {0, 1, 2, 3, 4, 5}, {1, 2, 3, 4}, {9}]
    units, levels, sets = br.mine(members, 5, 4)
    assert [(s['units'][:2], s['works'], s['closed']) for s in sets] == [([0, 1], 5, 1)]
    assert levels[0]['candidates'] == 1 and units[2] == dict(works=4, sets=0, largest=0)
    units, levels, sets = br.mine(members, 4, 4)              # unit 2 exactly at the bar
    assert [s['units'][:s['size']] for s in sets] == [[0, 1], [0, 2], [1, 2], [0, 1, 2]]
    assert [s['closed'] for s in sets] == [1, 0, 0, 1]        # (0, 1) has a work more
    assert [s['first_work'] for s in sets] == [0, 1, 1, 1]
    units, levels, sets = br.mine(members + [{9, 4}], 1, 2)   # one work is enough
    got = {tuple(s['units'][:2]): s['works'] for s in sets}
    assert got[(3, 4)] == 1 and got[(0, 4)] == 1 and (0, 3) not in got
    assert levels[0]['candidates'] == 10
    with pytest.raises(ValueError):
        br.mine(members, 0, 4)
    for k in (1, 9):
        with pytest.raises(ValueError):
            br.mine(members, 1, k)


def test_the_cap_names_the_level_and_the_count():
    members = [set(range(3)) for _ in range(6)]
    with pytest.raises(br.TooManySets) as e:
        br.mine(members, 1, 4, max_sets=19)                   # level 3: C(6, 3) = 20
    assert (e.value.level, e.value.count) == (3, 20)
    with pytest.raises(br.TooManySets) as e:
        br.mine(members, 1, 4, max_sets=14)                   # level 2: 15 kept pairs
    assert (e.value.level, e.value.count) == (2, 15)
    assert len(br.mine(members, 1, 4, max_sets=20)[2]) == 15 + 20 + 15


def test_lift_of_a_set_of_eight_at_two_to_the_twenty_works():
    """N ** 7 = 2^140: Python integers need no guard, and the product's code must stay in them
    whatever it is handed."""
    n = 1 << 20
    ws = [3, 5, 7, 11, 13, 17, 19, 23]
    want = 2 * n ** 7 * 1000 // (3 * 5 * 7 * 11 * 13 * 17 * 19 * 23)
    assert want > 1 << 64
    assert br.lift_permille(2, n, ws) == want
    assert bundles.lift_permille(2, n, ws) == want
    got = bundles.lift_permille(np.uint32(2), np.uint32(n), np.array(ws, dtype=np.uint32))
    assert got == want and type(got) is int
    assert bundles.lift_permille(np.uint32(40), np.int64(50), [np.uint32(40)] * 2) == 1250
    assert bundles.lift_permille(n, n, [n, n]) == 1000        # independent quoting


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["bundles", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_bundles"
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.min_all,
            args.max_size, args.all, args.device, args.reader) == \
        (None, "region", 6, 0, 1, 5, 4, False, 0, None)
    assert bundles.output_names(args.matches) == (
        "runs/match-6gram-20240101-bundles.csv", "runs/match-6gram-20240101-bundles-units.csv",
        "runs/match-6gram-20240101-bundles-levels.csv")
    assert bundles.output_names("m.csv", "out/x")[2] == "out/x-bundles-levels.csv"
    args = cli.ao3_parser().parse_args(
        ["bundles", "m.csv", "-o", "p", "--by", "scene", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--min-all", "7", "--max-size", "8", "--all", "--device", "1",
         "--reader", "python"])
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.min_all,
            args.max_size, args.all, args.device, args.reader) == \
        ("p", "scene", 3, 2, 4, 7, 8, True, 1, "python")
    assert (bundles.SET_FIELDS, bundles.UNIT_FIELDS, bundles.LEVEL_FIELDS) == \
        (br.SET_FIELDS, br.UNIT_FIELDS, br.LEVEL_FIELDS)
    assert "bundles" in cli.ao3_parser().format_help()
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["bundles", "m.csv", "--by", "word"])


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--min-all", "0"],
                                 ["--max-size", "1"], ["--max-size", "9"], ["--max-gap", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["bundles", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py bundles: error: ")
    assert "\n" not in str(e.value.code)


def test_a_refused_level_is_one_error_line(monkeypatch, tmp_path):
    def refuse(*a, **k):
        raise _lib.FsError(abi.FS_E_UNSUPPORTED, "fs_bundles",
                           "bundles: level 3 has 20 candidate sets, more than 19")
    monkeypatch.setattr(bundles, "find_bundles", refuse)
    monkeypatch.setattr(bundles, "units_of", lambda *a: (np.zeros(0, np.uint32), []))
    with pytest.raises(SystemExit) as e:
        cli.main(["bundles", os.path.join(GOLDEN, mbg.CONTRAST), "-o", str(tmp_path / "p"),
                  "--reader", "python"])
    line = str(e.value.code)
    assert line.startswith("ao3.py bundles: error: ") and "level 3 has 20" in line
    assert "\n" not in line and not os.listdir(str(tmp_path))  # before anything is written


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_bundles", "fs_bundles_rows", "fs_bundles_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "bundles" in _lib.TIMED
    for name, value in (("FS_BUNDLES_MAX_SIZE", "8u"), ("FS_BUNDLES_MAX_SETS", "(1u << 22)"),
                        ("FS_BUNDLES_MAX_BYTES", "(1u << 30)"), ("FS_BUNDLES_TIMES", "32")):
        assert "#define %s %s\n" % (name, value) in text
    assert (abi.FS_BUNDLES_MAX_SIZE, abi.FS_BUNDLES_MAX_SETS, abi.FS_BUNDLES_MAX_BYTES,
            abi.FS_BUNDLES_TIMES) == (8, 1 << 22, 1 << 30, 32) == \
        (br.MAX_SIZE, br.MAX_SETS, 1 << 30, 32)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert "fs_bundles" in fh.read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_bundle", "BUNDLE_DTYPE", br.SET_KEYS + ["reserved"], 64),
    ("fs_bundle_unit", "BUNDLE_UNIT_DTYPE", br.UNIT_KEYS + ["reserved"], 16),
    ("fs_bundle_level", "BUNDLE_LEVEL_DTYPE", ["size", "frequent", "candidates", "closed",
                                               "maximal"], 24)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for kind, names in re.findall(r"uint(32|64)_t\s+([^;]+);", body):
        for n in names.split(","):
            name, count = re.match(r"\s*(\w+)(?:\[(\d+)\])?", n).groups()
            fields.append((name, at))
            at += int(kind) // 8 * int(count or 1)
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    got = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    units = np.ones(2, dtype=abi.BUNDLE_UNIT_DTYPE)
    levels = np.ones(8, dtype=abi.BUNDLE_LEVEL_DTYPE)
    found = np.ones(4, dtype=abi.BUNDLE_DTYPE)
    up, lp, fp = (x.ctypes.data_as(C.c_void_p) for x in (units, levels, found))

    def call(n_rows=1, n_script=4, unit_of=u32, n_units=2, min_words=1, min_all=1, max_size=4,
             out=up, lev=lp, sets=fp, cap=4, n_out=C.byref(got), cols=u32):
        return L.fs_bundles(0, cols, cols, cols, n_rows, 1, n_script, unit_of, n_units,
                            min_words, 0, min_all, max_size, out, lev, sets, cap, n_out)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_all=0) == abi.FS_E_INVALID
    assert call(max_size=1) == abi.FS_E_INVALID
    assert call(max_size=9) == abi.FS_E_INVALID
    assert b"2 to 8" in L.fs_last_error()
    assert call(out=None) == abi.FS_E_INVALID
    assert call(lev=None) == abi.FS_E_INVALID
    assert call(sets=None) == abi.FS_E_INVALID                # a capacity without a buffer
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["works"] == 1).all() and (levels["size"] == 1).all()   # nothing written
    # no records, and no units: units nobody quotes and empty levels, no device work
    assert call(n_rows=0, cols=None, unit_of=None, sets=None, cap=0, max_size=3) == abi.FS_OK
    assert got.value == 0
    assert [tuple(u) for u in units.tolist()] == [(0, 0, 0, 0)] * 2
    assert [tuple(v) for v in levels.tolist()[:3]] == [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0),
                                                       (4, 0, 0, NONE, NONE)]
    assert levels["size"][3] == 1                             # max_size records, no more
    got.value = 7
    assert call(n_units=0, out=None, unit_of=None) == abi.FS_OK and got.value == 0
    assert (found["works"] == 1).all()
    assert L.fs_bundles_times(None) == abi.FS_E_INVALID
    assert L.fs_bundles_rows(None, None, 0, 0, None, 0, 1, 0, 1, 4, None, None, None, 0,
                             C.byref(got)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        bundles.find_bundles(z, z, z, 1, 5, z, 1)             # a map of 4 entries for 5 words


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, min_all=5, max_size=4, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    units, levels, sets = br.bundles(recs, n_works, n_script, np.asarray(unit_of).tolist(),
                                     n_units, min_words, max_gap, min_all, max_size)
    return as_records(units, levels, sets)


def as_records(units, levels, sets):
    """The dicts of the restatement as the library's records."""
    u = np.zeros(len(units), dtype=abi.BUNDLE_UNIT_DTYPE)
    for name in br.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    v = np.zeros(len(levels), dtype=abi.BUNDLE_LEVEL_DTYPE)
    for name in br.LEVEL_KEYS:
        v[name] = [d[name] for d in levels]
    s = np.zeros(len(sets), dtype=abi.BUNDLE_DTYPE)
    for name in br.SET_KEYS:
        if len(sets):
            s[name] = [d[name] for d in sets]
    return u, v, s


def test_the_golden_generator_reproduces_its_committed_files():
    made = mbg.build()
    assert set(made) == {n for c in mbg.CASES for n in mbg.golden_names(c[0], c[1])}
    assert len(made) == 15
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("source,case,by,min_words,max_gap,min_works,min_all,max_size,every",
                         mbg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, source, case, by, min_words,
                                                      max_gap, min_works, min_all, max_size,
                                                      every):
    from fandom_search_amd import companions
    monkeypatch.setattr(bundles, "find_bundles", oracle_find)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    body = bundles.tables(read_matches(os.path.join(GOLDEN, source)), by, min_words, max_gap,
                          min_works, min_all, max_size, every)
    heads = (bundles.SET_FIELDS, bundles.UNIT_FIELDS, bundles.LEVEL_FIELDS)
    for name, head, part in zip(mbg.golden_names(source, case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_goldens_hold_what_the_fixtures_are_known_to_hold():
    made = mbg.build()

    def table(source, case, kind):
        text = made[mbg.golden_names(source, case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    # frequent sets by size, as counted on the fixtures before the command existed
    assert [r[2] for r in table(mbg.CONTRAST, "all2", 2)] == ["17", "15", "4", "0"]
    assert [r[2] for r in table(mbg.CONTRAST, "default", 2)] == ["10", "3", "0", "0", "0"][:4]
    deep = table(mbg.RETELLINGS, "deep", 2)
    assert [r[2] for r in deep] == ["15", "20", "15", "6", "1", "0", "0", "0"]
    assert deep[-1][3:5] == ["", ""] and deep[4][3:6] == ["1", "1", "1"]
    assert len(table(mbg.CONTRAST, "all2", 0)) == 36           # --all prints every set
    sets = table(mbg.CONTRAST, "default", 0)
    assert all(r[7] == "1" for r in sets)                      # closed only
    assert [int(r[3]) for r in sets] == sorted((int(r[3]) for r in sets), reverse=True)
    assert [r[0] for r in sets] == [str(k + 1) for k in range(len(sets))]
    size3 = table(mbg.RETELLINGS, "gap1_size3", 0)
    assert {r[1] for r in size3} == {"2", "3"}
    assert any(r[1] == "3" and r[7] == "0" and int(r[8]) > 0 for r in size3)   # marked by level 4
    assert table(mbg.RETELLINGS, "gap1_size3", 2)[2][3:6] == ["", "", "0"]
    scene = table(mbg.CONTRAST, "scene", 0)
    assert scene and all(r[13] == "" and r[11].replace(" | ", "") == "" for r in scene)
