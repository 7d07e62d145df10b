"""`ao3.py saturation` without a GPU: the hash, the bucket of a time and the invariants of the
restated contract (tests/saturation_restated.py), the draw held to the distribution it claims,
the Chao2 arithmetic, the parser, the C ABI's declarations, and the committed expected CSVs
under the product's table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import math
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, companions, saturation
from fandom_search_amd.passages import read_matches
from tests import intervals_restated as ir
from tests import saturation_restated as sr
from tests.golden import make_saturation_golden as msg
from tests.test_companions_host import oracle_quotes, works_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF
POINTS = (1, 2, 3, 7, 10, 1000, 1024)


# ---- the hash and the bucket ---------------------------------------------------------------

def test_hash_known_answers_shared_with_intervals():
    known = [((0, 0, 0), 0), ((1, 0, 0), 0xE220A839), ((0, 0, 1), 0x5692161D),
             ((0, 4095, 0xFFFFFFFF), 0x3C02895C), ((2 ** 64 - 1, 4095, 0xFFFFFFFF), 0x91144CFF)]
    for args, want in known:
        assert sr.hash32(*args) == ir.hash32(*args) == want
    rs, ws = [0, 1, 63, 64, 4095], [0, 1, 63, 64, 31243, 2 ** 28 - 1, 2 ** 32 - 1]
    for seed in (0, 1, 7, 2 ** 63 + 12345, 2 ** 64 - 1):
        got = sr.hash_np(seed, rs, ws)
        assert got.tolist() == [[sr.hash32(seed, r, w) for w in ws] for r in rs]
        assert got.tolist() == [[ir.hash32(seed, r, w) for w in ws] for r in rs]


@pytest.mark.parametrize("K", POINTS)
def test_bucket_is_the_first_point_that_holds_the_time(K):
    L = _lib.load()
    assert sr.threshold(K, K) == 2 ** 32 and sr.threshold(0, K) == 0
    for h, want in ((0, 1), (2 ** 32 - 1, K)):
        assert sr.bucket_by_definition(h, K) == sr.bucket(h, K) == want
        assert L.fs_saturation_bucket(h, K) == want
    for c in range(1, K + 1):
        T = sr.threshold(c, K)
        assert T > sr.threshold(c - 1, K)
        # the last time inside point c, and the first that is not
        for h, want in ((T - 1, c), (T, c + 1)):
            if h == 2 ** 32:
                continue
            assert sr.bucket_by_definition(h, K) == want, (h, K)
            assert sr.bucket(h, K) == want, (h, K)
            assert L.fs_saturation_bucket(h, K) == want, (h, K)


# ---- invariants of the restatement ---------------------------------------------------------

def small_case():
    """Seven works over a script of 40 words: work 3 has three stray words and is not active;
    unit 4 is quoted by nobody, unit 2 by one work, unit 3 by two."""
    recs = works_of([[(0, 6), (10, 6)], [(0, 6)], [(10, 6), (20, 6)], [(33, 3)], [(0, 6)],
                     [(26, 6), (0, 6)], [(26, 6)]])
    unit_of = [0] * 10 + [1] * 10 + [2] * 6 + [3] * 6 + [NONE] + [4] * 7
    return recs, 7, 40, unit_of, 5


@pytest.mark.parametrize("K,R,level", [(1, 1, 95), (2, 5, 50), (7, 33, 99), (100, 16, 95)])
def test_the_curves_rise_and_end_at_everything(K, R, level):
    recs, n_works, n_script, unit_of, n_units = small_case()
    works, pts, perms, summary, first = sr.saturation(recs, n_works, n_script, unit_of, n_units,
                                                      permutations=R, points=K, seed=5,
                                                      level=level)
    assert works == [4, 2, 1, 2, 0]
    assert summary == dict(n_active=6, units_quoted=4, singletons=1, doubletons=2)
    assert list(pts[0]) == sr.POINT_KEYS and list(perms[0]) == sr.PERM_KEYS
    assert len(pts) == K and len(perms) == R and len(first) == n_units
    assert first[4] == [NONE] * R and all(x != NONE for u in range(4) for x in first[u])
    for key in sr.POINT_KEYS:
        col = [p[key] for p in pts]
        assert col == sorted(col), key                       # monotone in c
    last = pts[-1]
    assert [last[k] for k in sr.POINT_KEYS[:5]] == [4] * 5 and last["units_sum"] == 4 * R
    assert [last[k] for k in sr.POINT_KEYS[5:8]] == [7] * 3 and last["works_sum"] == 7 * R
    for p in pts:
        assert p["units_min"] <= p["units_low"] <= p["units_median"] <= p["units_high"] \
            <= p["units_max"]
        assert p["works_low"] <= p["works_median"] <= p["works_high"]
    for v in perms:
        assert 1 <= v["half_at"] <= v["ninety_at"] <= v["all_at"] <= K
    # the first time of a unit is the smallest time of its works, whatever their active number
    active = [0, 1, 2, 4, 5, 6]
    for r in range(R):
        assert first[2][r] == sr.hash32(5, r, 2)
        assert first[0][r] == min(sr.hash32(5, r, w) for w in (0, 1, 4, 5))
        assert first[3][r] == min(sr.hash32(5, r, w) for w in active[4:])
    assert sr.saturation(recs, n_works, n_script, unit_of, n_units, permutations=R, points=K,
                         seed=5, level=level, fast=True) == (works, pts, perms, summary, first)


def test_nothing_quoted_and_the_refusals_of_the_restatement():
    recs, n_works, n_script, unit_of, n_units = small_case()
    works, pts, perms, summary, first = sr.saturation(recs, n_works, n_script, unit_of, n_units,
                                                      min_words=7, permutations=9, points=4)
    assert works == [0] * 5 and summary == dict(n_active=0, units_quoted=0, singletons=0,
                                                doubletons=0)
    assert perms == [dict(half_at=1, ninety_at=1, all_at=1)] * 9           # Q = 0
    assert all(p["units_max"] == 0 and p["units_sum"] == 0 for p in pts)
    assert pts[-1]["works_low"] == 7 and pts[0]["works_sum"] > 0         # the works are drawn
    assert first == [[NONE] * 9] * 5
    none = sr.saturation([], 0, 0, [], 0, permutations=2, points=3)
    assert none[0] == [] and none[2] == [dict(half_at=1, ninety_at=1, all_at=1)] * 2
    assert all(p == dict.fromkeys(sr.POINT_KEYS, 0) for p in none[1]) and none[4] == []
    for bad in (dict(min_words=0), dict(permutations=0), dict(permutations=4097),
                dict(points=0), dict(points=1025), dict(level=49), dict(level=100),
                dict(seed=2 ** 64), dict(seed=-1)):
        with pytest.raises(ValueError):
            sr.saturation(recs, n_works, n_script, unit_of, n_units, **bad)


# ---- the draw is what it claims ------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_a_unit_of_d_works_is_seen_with_the_probability_of_independent_draws(d, seed):
    """One unit quoted by d of 10 works, R = 4096 orders, K = 10 points: every work is in the
    sample at point c independently with probability c / K, so the unit has been seen with
    probability p = 1 - (1 - c / K)^d, and the orders in which it has lie within four standard
    deviations sqrt(R p (1 - p)) of R p.  The inputs are fixed, so the test is deterministic:
    with works 0 .. d - 1 the quoting ones the restated hash gives 1.85 at the most."""
    R, K = 4096, 10
    recs = works_of([[(0, 6)] if w < d else [(10, 3)] for w in range(10)])
    _, pts, _, summary, first = sr.saturation(recs, 10, 20, [0] * 6 + [NONE] * 14, 1,
                                              permutations=R, points=K, seed=seed, fast=True)
    assert summary["n_active"] == d and summary["units_quoted"] == 1
    worst = 0.0
    for c in range(1, K):
        seen = sum(1 for r in range(R) if first[0][r] < sr.threshold(c, K))
        assert seen == pts[c - 1]["units_sum"]
        p = 1 - (1 - c / K) ** d
        z = abs(seen - R * p) / math.sqrt(R * p * (1 - p))
        worst = max(worst, z)
        print("d", d, "seed", seed, "c", c, "seen", seen, "expected", R * p, "z", z)
        assert z <= 4
    assert worst <= 4


# ---- the summary's arithmetic ---------------------------------------------------------------

def test_chao2_in_integers():
    for f in (sr.unseen_estimate, saturation.unseen_estimate):
        assert f(32, 0, 0) == 0 and f(32, 1, 0) == 0           # Q1 (Q1 - 1) = 0
        assert f(10, 4, 1) == (9 * 4 * 3) // (10 * 2 * 2) == 2
        assert f(1, 5, 0) == 0                                 # one work: n - 1 = 0
        assert f(1000, 300, 0) == (999 * 300 * 299) // 2000 == 44805
        big = f(2 ** 28, 2 ** 19, 0)                           # past 64 bits on the way
        assert big == ((2 ** 28 - 1) * 2 ** 19 * (2 ** 19 - 1)) // (2 ** 29)
        assert f(0, 0, 0) == 0


# ---- product side that needs no GPU --------------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["saturation", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_saturation"
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works,
            args.permutations, args.points, args.seed, args.level, args.device, args.reader) == \
        (None, "word", 6, 0, 1, 1000, 100, 0, 95, 0, None)
    assert saturation.output_names(args.matches) == (
        "runs/match-6gram-20240101-saturation.csv",
        "runs/match-6gram-20240101-saturation-permutations.csv",
        "runs/match-6gram-20240101-saturation-summary.csv")
    assert saturation.output_names("m.csv", "out/x")[2] == "out/x-saturation-summary.csv"
    args = cli.ao3_parser().parse_args(
        ["saturation", "m.csv", "-o", "p", "--by", "scene", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--permutations", "64", "--points", "1024", "--seed",
         str(2 ** 64 - 1), "--level", "90", "--device", "1", "--reader", "python"])
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works,
            args.permutations, args.points, args.seed, args.level, args.device, args.reader) == \
        ("p", "scene", 3, 2, 4, 64, 1024, 2 ** 64 - 1, 90, 1, "python")
    for by in ("scene", "character", "region", "word"):
        assert cli.ao3_parser().parse_args(["saturation", "m", "--by", by]).by == by
    assert saturation.POINT_FIELDS == sr.POINT_FIELDS
    assert saturation.PERMUTATION_FIELDS == sr.PERMUTATION_FIELDS
    assert saturation.SUMMARY_FIELDS == sr.SUMMARY_FIELDS
    text = cli.ao3_parser().format_help()
    assert "contrast, saturation or validate" in " ".join(text.split())
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["saturation", "m.csv", "--by", "line"])
    # the parsers the other tests pin do not know the command
    for parser in (cli.build_parser(), cli.full_parser()):
        with pytest.raises(SystemExit):
            parser.parse_args(["saturation", "m.csv"])


@pytest.mark.parametrize("bad,message", [
    (["--min-words", "0"], "--min-words and --min-works must be at least 1, --max-gap at least 0"),
    (["--min-works", "0"], "--min-words and --min-works must be at least 1, --max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words and --min-works must be at least 1, --max-gap at least 0"),
    (["--permutations", "0"], "--permutations must be from 1 to 4096"),
    (["--permutations", "4097"], "--permutations must be from 1 to 4096"),
    (["--points", "0"], "--points must be from 1 to 1024"),
    (["--points", "1025"], "--points must be from 1 to 1024"),
    (["--level", "49"], "--level must be from 50 to 99"),
    (["--level", "100"], "--level must be from 50 to 99"),
    (["--seed", "-1"], "--seed must be from 0 to 2^64 - 1"),
    (["--seed", str(2 ** 64)], "--seed must be from 0 to 2^64 - 1")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["saturation", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py saturation: error: " + message


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_saturation", "fs_saturation_rows", "fs_saturation_times",
                 "fs_saturation_bucket"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "saturation" in _lib.TIMED
    assert abi.SATURATION_MS_NAMES == ("incidence", "sizes", "times", "product", "curve",
                                       "points", "total", "table", "ksplit", "osplit")
    assert re.search(r"#define FS_SATURATION_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_SATURATION_MAX_WORKS \(1u << 28\)", text)
    assert re.search(r"#define FS_SATURATION_MAX_PERMUTATIONS 4096u", text)
    assert re.search(r"#define FS_SATURATION_MAX_POINTS 1024u", text)
    assert (abi.FS_SATURATION_MAX_BYTES, abi.FS_SATURATION_MAX_WORKS,
            abi.FS_SATURATION_MAX_PERMUTATIONS, abi.FS_SATURATION_MAX_POINTS) == \
        (1 << 30, 1 << 28, 4096, 1024)
    # one copy of the hash, in the shared header, and one of the sort
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    body = open(os.path.join(src, "fs_saturation.hip")).read()
    assert "fs_work_hash(" in body and "0xBF58476D1CE4E5B9" not in body
    assert open(os.path.join(src, "fs_hash.h")).read().count("0xBF58476D1CE4E5B9") == 1
    for unit in ("fs_saturation.hip", "fs_intervals.hip"):
        assert "block_sort_two<" in open(os.path.join(src, unit)).read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_saturation_point", "SATURATION_POINT_DTYPE",
     sr.POINT_KEYS + ["reserved0", "reserved1"], 64),
    ("fs_saturation_perm", "SATURATION_PERM_DTYPE", sr.PERM_KEYS + ["reserved"], 16),
    ("fs_saturation_summary", "SATURATION_SUMMARY_DTYPE", sr.SUMMARY_KEYS, 16)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for bits, names in re.findall(r"uint(32|64)_t\s+([^;]+);", body):
        for n in names.split(","):
            at = (at + int(bits) // 8 - 1) // (int(bits) // 8) * (int(bits) // 8)
            fields.append((n.strip(), at, int(bits) // 8))
            at += int(bits) // 8
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at and size & (size - 1) == 0
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    works = np.ones(2, dtype=np.uint32)
    pts = np.zeros(4, dtype=abi.SATURATION_POINT_DTYPE)
    pts["units_low"] = 1
    perms = np.ones(16, dtype=np.uint32).view(abi.SATURATION_PERM_DTYPE)
    summary = np.ones(4, dtype=np.uint32).view(abi.SATURATION_SUMMARY_DTYPE)
    wp, pp, rp, sp = (x.ctypes.data_as(C.c_void_p) for x in (works, pts, perms, summary))
    assert len(perms) == 4 and len(summary) == 1

    def call(n_rows=1, n_works=1, n_script=4, unit_of=u32, n_units=2, min_words=1,
             permutations=4, points=4, level=95, out_works=wp, out_pts=pp, out_perms=rp,
             out_summary=sp, cols=u32):
        return L.fs_saturation(0, cols, cols, cols, n_rows, n_works, n_script, unit_of, n_units,
                               min_words, 0, permutations, points, 0, level, out_works, out_pts,
                               out_perms, out_summary, None)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert b"records: saturation curves take fewer than 2^32" in L.fs_last_error()
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(n_works=(1 << 28) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    for permutations in (0, 4097):
        assert call(permutations=permutations) == abi.FS_E_INVALID
    for points in (0, 1025):
        assert call(points=points) == abi.FS_E_INVALID
    for level in (49, 100):
        assert call(level=level) == abi.FS_E_INVALID
    for name in ("out_works", "out_pts", "out_perms", "out_summary", "unit_of", "cols"):
        assert call(**{name: None}) == abi.FS_E_INVALID, name
    assert (works == 1).all() and (perms["half_at"] == 1).all()           # nothing written
    assert (summary["units_quoted"] == 1).all()
    assert L.fs_saturation_times(None) == abi.FS_E_INVALID
    assert L.fs_saturation_rows(None, None, 0, 0, None, 0, 1, 0, 4, 4, 0, 95, None, None, None,
                                None, None) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        saturation.find_saturation(z, z, z, 1, 5, z, 1)        # a map of 4 entries for 5 words
    with pytest.raises(ValueError):
        saturation.find_saturation(z, z, z, 1, 4, z, 1, seed=1 << 64)


# ---- committed expected outputs ------------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, permutations=1000, points=100, seed=0, level=95, first=False,
                device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    works, pts, perms, summary, _ = sr.saturation(
        recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units, min_words, max_gap,
        permutations, points, seed, level)
    p = np.zeros(len(pts), dtype=abi.SATURATION_POINT_DTYPE)
    for k in sr.POINT_KEYS:
        p[k] = [d[k] for d in pts]
    r = np.zeros(len(perms), dtype=abi.SATURATION_PERM_DTYPE)
    for k in sr.PERM_KEYS:
        r[k] = [d[k] for d in perms]
    s = np.zeros(1, dtype=abi.SATURATION_SUMMARY_DTYPE)
    for k in sr.SUMMARY_KEYS:
        s[k] = summary[k]
    return np.array(works, dtype=np.uint32), p, r, s


def test_the_golden_generator_reproduces_its_committed_files():
    made = msg.build()
    assert set(made) == {n for c in msg.CASES for n in msg.golden_names(c[0])}
    assert msg.INPUT not in made                               # read, never written
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,by,min_words,max_gap,min_works,permutations,points,seed,level",
                         msg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, by, min_words, max_gap,
                                                      min_works, permutations, points, seed,
                                                      level):
    monkeypatch.setattr(saturation, "find_saturation", oracle_find)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    body = saturation.tables(read_matches(os.path.join(GOLDEN, msg.INPUT)), by, min_words,
                             max_gap, min_works, permutations, points, seed, level)
    heads = (saturation.POINT_FIELDS, saturation.PERMUTATION_FIELDS, saturation.SUMMARY_FIELDS)
    for name, head, part in zip(msg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_goldens_hold_what_the_cases_say():
    made = msg.build()

    def table(case, kind):
        text = made[msg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    assert msg.CASES[0][1:] == ("word", 6, 0, 1, 1000, 100, 0, 95)        # the defaults
    curve = table("default", 0)
    assert len(curve) == 100 and len(table("default", 1)) == 1000
    assert [r[0] for r in curve] == [str(c) for c in range(1, 101)]
    assert curve[9][1] == "100000" and curve[-1][1] == "1000000"
    assert curve[-1][2:5] == ["32", "32", "32"] and curve[-1][5] == "32000"
    summary = table("default", 2)
    assert len(summary) == 1 and summary[0][:4] == ["32", "26", "25", "25"]
    assert curve[-1][6:11] == ["25"] * 5 and curve[-1][12] == "100"
    assert int(curve[0][13]) > int(curve[49][13]) >= int(curve[-1][13]) == 0   # it flattens
    for c, r in enumerate(curve[1:], 1):
        assert int(r[5]) >= int(curve[c - 1][5]) and int(r[11]) >= int(curve[c - 1][11])
    scene = table("scene", 2)[0]
    assert scene[2:4] == ["4", "3"]                            # a scene nobody quotes
    assert len(table("scene", 0)) == 10 and len(table("scene", 1)) == 64
    assert table("scene", 0)[-1][6:11] == ["3"] * 5
    region = table("region_gap1", 2)[0]
    assert region[1:4] == ["27", "5", "5"]                     # the fifth line under --max-gap 1
    assert len(table("region_gap1", 0)) == 7 and len(table("region_gap1", 1)) == 40
    assert [r[1] for r in table("region_gap1", 0)][:2] == ["142857", "285714"]
    for case in ("default", "scene", "region_gap1"):
        for row in table(case, 1):
            assert int(row[1]) <= int(row[2]) <= int(row[3]) <= 1000000
