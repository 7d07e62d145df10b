"""`routes` without a GPU: the restated contract (tests/routes_restated.py) against a brute
force over all index tuples of every work, hand-made answers, the CSV formatting, the command
line, the ABI, and the committed expected outputs."""

import csv
import ctypes as C
import io
import itertools
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, routes
from fandom_search_amd.passages import read_matches
from tests import routes_restated as rr
from tests.golden import make_routes_golden as mrg
from tests.test_companions_host import oracle_quotes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = rr.NONE


# ---- the restatement against a brute force ----------------------------------------------

def brute(seqs, n_units, max_skip, min_all, max_length):
    """Every index tuple of every work of two or more elements taken directly, no levels and no
    dynamic programme: {route: sorted supporting works} of the frequent ones of 2 ..
    max_length + 1 units."""
    reach = None if max_skip == NONE else max_skip + 1
    found = {}
    for w, s in seqs.items():
        if len(s) < 2:
            continue
        mine = set()
        for k in range(2, max_length + 2):
            for at in itertools.combinations(range(len(s)), k):
                if reach is None or all(q - p <= reach for p, q in zip(at, at[1:])):
                    r = tuple(s[p] for p in at)
                    if all(a != b for a, b in zip(r, r[1:])):
                        mine.add(r)
        for r in mine:
            found.setdefault(r, []).append(w)
    return {r: sorted(ws) for r, ws in found.items() if len(ws) >= min_all}


def random_sequences(rng, n_units, n_works, longest):
    return {w: rr.collapse(rng.integers(0, n_units, size=int(rng.integers(0, longest + 1))).tolist())
            for w in range(n_works)}


@pytest.mark.parametrize("seed", range(10))
def test_the_level_wise_restatement_equals_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    n_units = int(rng.integers(2, 5))
    seqs = random_sequences(rng, n_units, int(rng.integers(1, 14)), 7)
    returning = 0
    for max_skip in (NONE, 0, 1, 3):
        for min_all, max_length in ((1, 2), (2, 3), (1, 4), (3, 3)):
            freq = brute(seqs, n_units, max_skip, min_all, max_length)
            units, levels, found = rr.mine(seqs, n_units, max_skip, min_all, max_length)
            got = {tuple(r['units'][:r['length']]): r for r in found}
            assert set(got) == {r for r in freq if len(r) <= max_length}
            order = [(r['length'], r['units'][:r['length']]) for r in found]
            assert order == sorted(order)                      # by length, then lexicographic
            for r, rec in got.items():
                assert rec['works'] == len(freq[r]) and rec['first_work'] == freq[r][0]
                assert rec['units'][len(r):] == [NONE] * (8 - len(r))
                ahead = [t for t in freq if t[:-1] == r]
                behind = [t for t in freq if t[1:] == r]
                assert (rec['forward'], rec['backward']) == (len(ahead), len(behind))
                assert rec['closed'] == int(all(len(freq[t]) != len(freq[r])
                                                for t in ahead + behind))
                returning += len(set(r)) < len(r)
            long_works = [s for s in seqs.values() if len(s) >= 2]
            for u, v in enumerate(units):
                holding = [r for r in got if u in r]
                assert v == dict(works=sum(u in s for s in long_works), routes=len(holding),
                                 longest=max([len(r) for r in holding], default=0))
            for r, rec in got.items():
                before = units[r[0]]['works'] if len(r) == 2 else len(freq[r[:-1]])
                assert rec['prefix_works'] == before
            assert [v['length'] for v in levels] == list(range(2, max_length + 2))
            single = sum(1 for v in units if v['works'] >= min_all)
            assert levels[0]['candidates'] == single * (single - 1)
            for v in levels:
                k = v['length']
                assert v['frequent'] == sum(1 for r in freq if len(r) == k) <= v['candidates']
                want = NONE if k > max_length else sum(rec['closed'] for rec in found
                                                       if rec['length'] == k)
                assert v['closed'] == want
    assert returning > 0 or n_units > 3                        # (a, b, a) is a route


def test_support_at_the_skip_bound_and_one_beyond():
    seq = [0, 2, 3, 2, 1]                                      # 0 and 1 are four apart
    assert rr.supports(seq, (0, 1), NONE) and rr.supports(seq, (0, 1), 3)
    assert not rr.supports(seq, (0, 1), 2) and not rr.supports(seq, (0, 1), 0)
    assert rr.supports(seq, (0, 2, 1), 2) and not rr.supports(seq, (0, 2, 1), 1)
    assert not rr.supports(seq, (0, 3, 1), 0) and rr.supports(seq, (0, 3, 1), 1)
    assert rr.supports([0, 1, 0, 1], (0, 1, 0, 1), 0) and not rr.supports([0, 1, 0], (0, 1, 0, 1))
    assert rr.collapse([0, 0, 0, 1]) == [0, 1] and rr.collapse([]) == []


def test_a_planted_route_of_three_in_forty_works_and_what_closes_it():
    seqs = {w: [0, 1, 2] for w in range(40)}
    seqs.update({40: [1], 41: [2, 2 + 1], 42: []})
    units, levels, found = rr.mine(seqs, 4, NONE, 5, 4)
    assert [(r['units'][:r['length']], r['works'], r['closed']) for r in found] == \
        [([0, 1], 40, 0), ([0, 2], 40, 1), ([1, 2], 40, 0), ([0, 1, 2], 40, 1)]
    assert found[3]['prefix_works'] == 40 and found[0]['prefix_works'] == 40
    assert (found[0]['forward'], found[0]['backward']) == (1, 0)
    assert (found[2]['forward'], found[2]['backward']) == (0, 1)
    assert (found[1]['forward'], found[1]['backward']) == (0, 0)   # no contiguous part of it
    assert units[1] == dict(works=40, routes=3, longest=3)     # the work of one element: no part
    assert units[3] == dict(works=1, routes=0, longest=0)
    assert [(v['candidates'], v['frequent'], v['closed']) for v in levels] == \
        [(6, 3, 1), (1, 1, 1), (0, 0, 0), (0, 0, NONE)]
    units, levels, found = rr.mine(seqs, 4, 0, 5, 4)           # contiguous runs only
    assert [r['units'][:r['length']] for r in found] == [[0, 1], [1, 2], [0, 1, 2]]
    with pytest.raises(ValueError):
        rr.mine(seqs, 4, 64, 5, 4)
    for k in (1, 9):
        with pytest.raises(ValueError):
            rr.mine(seqs, 4, NONE, 5, k)
    with pytest.raises(rr.TooManyRoutes) as e:
        rr.mine(seqs, 4, NONE, 1, 4, max_sets=11)              # level 2: 4 * 3 ordered pairs
    assert (e.value.level, e.value.count) == (2, 12)


# ---- the formatting ---------------------------------------------------------------------

ABOUT = [(10, 12, "HAN", "4", "a b c"), (20, 21, "LEIA", "5", "d e"), (30, 30, "LUKE", "6", "f")]


def _records(units, levels, found):
    u = np.zeros(len(units), dtype=abi.ROUTE_UNIT_DTYPE)
    for name in rr.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    v = np.zeros(len(levels), dtype=abi.ROUTE_LEVEL_DTYPE)
    for name in rr.LEVEL_KEYS:
        v[name] = [d[name] for d in levels]
    s = np.zeros(len(found), dtype=abi.ROUTE_DTYPE)
    for name in rr.ROUTE_KEYS:
        if len(found):
            s[name] = [d[name] for d in found]
    return u, v, s


as_records = _records


def test_rows_from_hand_made_records(monkeypatch):
    seqs = {0: [2, 1, 0], 1: [2, 1, 0], 2: [0, 1, 0], 3: [1, 0]}
    mined = rr.mine(seqs, 3, NONE, 2, 3)
    names = ["w0.txt", "w1.txt", "w2.txt", "w3.txt"]
    want = rr.tables(*mined, ABOUT, names, "region", 3, False)
    monkeypatch.setattr(routes, "find_routes", lambda *a: _records(*mined))
    monkeypatch.setattr(routes, "units_of", lambda *a: (np.zeros(0, np.uint32), ABOUT))
    z = np.zeros(0, np.uint32)
    got = routes._tables(None, names, z, z, z, z, 0, "region", 6, 0, 1, 2, 3, None, False, 0)
    assert [ROW for ROW in got[0]] == want[0][1:] and got[1] == want[1][1:]
    assert got[2] == want[2][1:]
    rows = {r[2]: r for r in got[0]}
    assert rows["2 > 1"][3:10] == [4, 4, 100, "back", 1, 0, 1]
    assert rows["3 > 2 > 1"][3:10] == [2, 2, 100, "back", 1, 0, 0]
    assert rows["3 > 2 > 1"][10:] == ["w0.txt", "30 20 10", "LUKE | LEIA | HAN", "6 | 5 | 4",
                                      "f | d e | a b c"]
    assert "3 > 2" not in rows                                 # (3, 2) has the works of (3, 2, 1)
    assert [r[0] for r in got[0]] == list(range(1, len(got[0]) + 1))
    assert [r[3] for r in got[0]] == sorted((r[3] for r in got[0]), reverse=True)
    assert got[1][0][5:9] == [4, len([r for r in mined[2] if 0 in r['units']]), 3, 1]
    assert got[2][-1][3] == "" and got[2][0][4] == sum(1 for r in got[0] if r[1] == 2)
    every = routes._tables(None, names, z, z, z, z, 0, "scene", 6, 0, 1, 2, 3, None, True, 0)
    assert len(every[0]) == len(mined[2]) and all(r[14] == "" for r in every[0])
    assert routes.direction((0, 1, 2)) == "forward" and routes.direction((2, 0)) == "back"
    assert routes.direction((0, 1, 0)) == "mixed" == rr.direction([0, 2, 1])
    for bad in (dict(min_all=0), dict(max_length=1), dict(max_length=9), dict(max_skip=64),
                dict(max_skip=-1), dict(by="word")):
        opts = dict(by="region", min_all=2, max_length=3, max_skip=None)
        opts.update(bad)
        with pytest.raises(ValueError):
            routes._tables(None, names, z, z, z, z, 0, opts["by"], 6, 0, 1, opts["min_all"],
                           opts["max_length"], opts["max_skip"], False, 0)


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["routes", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_routes"
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.min_all,
            args.max_length, args.max_skip, args.all, args.device, args.reader) == \
        (None, "region", 6, 0, 1, 5, 4, None, False, 0, None)
    assert routes.output_names(args.matches) == (
        "runs/match-6gram-20240101-routes.csv", "runs/match-6gram-20240101-routes-units.csv",
        "runs/match-6gram-20240101-routes-levels.csv")
    assert routes.output_names("m.csv", "out/x")[2] == "out/x-routes-levels.csv"
    args = cli.ao3_parser().parse_args(
        ["routes", "m.csv", "-o", "p", "--by", "scene", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--min-all", "7", "--max-length", "8", "--max-skip", "0", "--all",
         "--device", "1", "--reader", "python"])
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.min_all,
            args.max_length, args.max_skip, args.all, args.device, args.reader) == \
        ("p", "scene", 3, 2, 4, 7, 8, 0, True, 1, "python")
    assert (routes.ROUTE_FIELDS, routes.UNIT_FIELDS, routes.LEVEL_FIELDS) == \
        (rr.ROUTE_FIELDS, rr.UNIT_FIELDS, rr.LEVEL_FIELDS)
    assert "routes" in cli.ao3_parser().format_help()
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["routes", "m.csv", "--by", "word"])


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--min-all", "0"],
                                 ["--max-length", "1"], ["--max-length", "9"],
                                 ["--max-gap", "-1"], ["--max-skip", "64"],
                                 ["--max-skip", "-1"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["routes", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py routes: error: ")
    assert "\n" not in str(e.value.code)


def test_a_refused_level_is_one_error_line(monkeypatch, tmp_path):
    def refuse(*a, **k):
        raise _lib.FsError(abi.FS_E_UNSUPPORTED, "fs_routes",
                           "routes: level 3 has 20 candidate routes, more than 19")
    monkeypatch.setattr(routes, "find_routes", refuse)
    monkeypatch.setattr(routes, "units_of", lambda *a: (np.zeros(0, np.uint32), []))
    with pytest.raises(SystemExit) as e:
        cli.main(["routes", os.path.join(GOLDEN, mrg.TRANSITIONS), "-o", str(tmp_path / "p"),
                  "--reader", "python"])
    line = str(e.value.code)
    assert line.startswith("ao3.py routes: error: ") and "level 3 has 20" in line
    assert "\n" not in line and not os.listdir(str(tmp_path))  # before anything is written


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_routes", "fs_routes_rows", "fs_routes_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "routes" in _lib.TIMED
    for name, value in (("FS_ROUTES_MAX_LENGTH", "8u"), ("FS_ROUTES_MAX_SKIP", "63u"),
                        ("FS_ROUTES_MAX_SETS", "(1u << 22)"),
                        ("FS_ROUTES_MAX_BYTES", "(1u << 30)"), ("FS_ROUTES_TIMES", "43")):
        assert "#define %s %s\n" % (name, value) in text
    assert (abi.FS_ROUTES_MAX_LENGTH, abi.FS_ROUTES_MAX_SKIP, abi.FS_ROUTES_MAX_SETS,
            abi.FS_ROUTES_MAX_BYTES, abi.FS_ROUTES_TIMES) == (8, 63, 1 << 22, 1 << 30, 43)
    assert (rr.MAX_LENGTH, rr.MAX_SKIP, rr.MAX_SETS) == (8, 63, 1 << 22)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        assert "fs_routes" in fh.read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_route", "ROUTE_DTYPE", rr.ROUTE_KEYS + ["reserved"], 64),
    ("fs_route_unit", "ROUTE_UNIT_DTYPE", rr.UNIT_KEYS + ["reserved"], 16),
    ("fs_route_level", "ROUTE_LEVEL_DTYPE", ["length", "frequent", "candidates", "closed",
                                             "reserved"], 24)])
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
    units = np.ones(2, dtype=abi.ROUTE_UNIT_DTYPE)
    levels = np.ones(8, dtype=abi.ROUTE_LEVEL_DTYPE)
    found = np.ones(4, dtype=abi.ROUTE_DTYPE)
    up, lp, fp = (x.ctypes.data_as(C.c_void_p) for x in (units, levels, found))

    def call(n_rows=1, n_script=4, unit_of=u32, n_units=2, min_words=1, max_skip=NONE,
             min_all=1, max_length=4, out=up, lev=lp, sets=fp, cap=4, n_out=C.byref(got),
             cols=u32):
        return L.fs_routes(0, cols, cols, cols, n_rows, 1, n_script, unit_of, n_units,
                           min_words, 0, max_skip, min_all, max_length, out, lev, sets, cap,
                           n_out)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_all=0) == abi.FS_E_INVALID
    assert call(max_length=1) == abi.FS_E_INVALID
    assert call(max_length=9) == abi.FS_E_INVALID
    assert b"2 to 8" in L.fs_last_error()
    assert call(max_skip=64) == abi.FS_E_INVALID
    assert call(max_skip=NONE - 1) == abi.FS_E_INVALID
    assert b"0 to 63" in L.fs_last_error()
    assert call(out=None) == abi.FS_E_INVALID
    assert call(lev=None) == abi.FS_E_INVALID
    assert call(sets=None) == abi.FS_E_INVALID                # a capacity without a buffer
    assert call(n_out=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["works"] == 1).all() and (levels["length"] == 1).all()   # nothing written
    # no records, and no units: units nobody quotes and empty levels, no device work
    for skip in (NONE, 0, 63):
        assert call(n_rows=0, cols=None, unit_of=None, sets=None, cap=0, max_length=3,
                    max_skip=skip) == abi.FS_OK
    assert got.value == 0
    assert [tuple(u) for u in units.tolist()] == [(0, 0, 0, 0)] * 2
    assert [tuple(v) for v in levels.tolist()[:3]] == [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0),
                                                       (4, 0, 0, NONE, 0)]
    assert levels["length"][3] == 1                           # max_length records, no more
    got.value = 7
    assert call(n_units=0, out=None, unit_of=None) == abi.FS_OK and got.value == 0
    assert (found["works"] == 1).all()
    assert L.fs_routes_times(None) == abi.FS_E_INVALID
    assert L.fs_routes_rows(None, None, 0, 0, None, 0, 1, 0, NONE, 1, 4, None, None, None, 0,
                            C.byref(got)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        routes.find_routes(z, z, z, 1, 5, z, 1)               # a map of 4 entries for 5 words


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, max_skip=None, min_all=5, max_length=4, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    return _records(*rr.routes(recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units,
                               min_words, max_gap, NONE if max_skip is None else max_skip,
                               min_all, max_length))


def test_the_golden_generator_reproduces_its_committed_files():
    made = mrg.build()
    assert set(made) == {n for c in mrg.CASES for n in mrg.golden_names(c[0], c[1])}
    assert len(made) == 15
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("source,case,by,min_words,max_gap,min_works,min_all,max_length,skip,"
                         "every", mrg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, source, case, by, min_words,
                                                      max_gap, min_works, min_all, max_length,
                                                      skip, every):
    from fandom_search_amd import companions
    monkeypatch.setattr(routes, "find_routes", oracle_find)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    body = routes.tables(read_matches(os.path.join(GOLDEN, source)), by, min_words, max_gap,
                         min_works, min_all, max_length, skip, every)
    heads = (routes.ROUTE_FIELDS, routes.UNIT_FIELDS, routes.LEVEL_FIELDS)
    for name, head, part in zip(mrg.golden_names(source, case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_goldens_hold_routes_of_three_units_and_a_returning_one():
    made = mrg.build()

    def table(source, case, kind):
        text = made[mrg.golden_names(source, case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    deep = table(mrg.RETELLINGS, "deep", 0)
    assert {r[1] for r in deep} == {"2", "3", "4"} and all(r[7] == "1" for r in deep)
    assert [r[0] for r in deep] == [str(k + 1) for k in range(len(deep))]
    assert [int(r[3]) for r in deep] == sorted((int(r[3]) for r in deep), reverse=True)
    assert all(r[2].count(" > ") == int(r[1]) - 1 for r in deep)
    assert [r[0] for r in table(mrg.RETELLINGS, "deep", 2)] == [str(k) for k in range(2, 10)]
    assert table(mrg.RETELLINGS, "deep", 2)[-1][3] == ""
    runs = table(mrg.TRANSITIONS, "run_all", 0)
    assert any(r[7] == "0" for r in runs) and any(r[1] == "3" for r in runs)
    scene = table(mrg.TRANSITIONS, "scene", 0)
    assert scene and all(r[14] == "" and r[12].replace(" | ", "") == "" for r in scene)
    assert len(table(mrg.TRANSITIONS, "default", 0)) == 1
