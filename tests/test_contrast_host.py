"""`ao3.py contrast` without a GPU: the restated contract (tests/contrast_restated.py) on an
example worked by hand and against the hypergeometric distribution, the exact square root of
the denominators, the sides, the parser, the C ABI's declarations, and the committed expected
CSVs under the product's table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import math
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, companions, contrast
from fandom_search_amd.passages import read_matches
from tests import contrast_restated as cn
from tests import groups_restated as gr
from tests.golden import make_contrast_golden as mcg
from tests.test_companions_host import oracle_quotes, works_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


# ---- an example small enough to check by hand ---------------------------------------------

def test_six_works_three_units_four_permutations_by_hand():
    """Units 0, 1, 2 are the script words 0-9, 10-19, 20-29.  Works 0, 2, 5 are side A, 1 and 4
    side B, 3 is out: N = 5, NA = 3.  Work 4 has three stray words and is not active.  At
    key_bits 0 side A of every permutation is the first three pool works, {0, 1, 2}."""
    recs = works_of([[(0, 6), (10, 6)], [(0, 6)], [(10, 6)], [(0, 6), (20, 6)], [(20, 3)],
                     [(0, 6), (10, 6), (20, 6)]])
    unit_of = [0] * 10 + [1] * 10 + [2] * 10
    side = [1, 2, 1, 0, 2, 1]
    units, perms, a_r = cn.contrast(recs, 6, 30, unit_of, 3, side, min_quoting=2, permutations=4,
                                    seed=9, key_bits=0)
    # unit 0: works 0, 1, 3, 5, of the pool 0, 1, 5: a = 2, b = 1, D = 2 * 5 - 3 * 3 = 1;
    #   den = isqrt(6 << 20) = 2508 (2508^2 = 6290064, 2509^2 = 6295081), X = 1048576 // 2508
    # unit 1: works 0, 2, 5: a = 3, b = 0, D = 15 - 9 = 6, X = 6291456 // 2508
    # unit 2: works 3, 5, of the pool 5: a = 1, b = 0, D = 5 - 3 = 2;
    #   den = isqrt(4 << 20) = 2048, X = 2097152 // 2048
    assert units == [dict(a_works=2, b_works=1, ge=4, adj_ge=4, statistic=418, d=1),
                     dict(a_works=3, b_works=0, ge=0, adj_ge=0, statistic=2508, d=6),
                     dict(a_works=1, b_works=0, ge=4, adj_ge=NONE, statistic=1024, d=2)]
    # every permutation: a_r = 2 (works 0, 1), 2 (works 0, 2), 0; D_r = 1, 1, -3; the family is
    # units 0 and 1, both at 1048576 // 2508 = 418, the first of them named
    assert a_r == [[2] * 4, [2] * 4, [0] * 4]
    assert perms == [dict(max_statistic=418, a_active=3, max_unit=0)] * 4
    assert list(units[0]) == cn.UNIT_KEYS and list(perms[0]) == cn.PERM_KEYS
    # min_quoting 1: unit 2 joins with X(-3) = 3145728 // 2048 = 1536, the largest
    units, perms, _ = cn.contrast(recs, 6, 30, unit_of, 3, side, min_quoting=1, permutations=4,
                                  key_bits=0)
    assert [u["adj_ge"] for u in units] == [4, 0, 4]
    assert perms == [dict(max_statistic=1536, a_active=3, max_unit=2)] * 4
    # the printed shares count the observed labelling as one permutation
    assert (4 + 1) * 1000000 // (4 + 1) == 1000000 and (0 + 1) * 1000000 // (4 + 1) == 200000


def test_ties_on_the_key_go_to_the_smaller_work_number():
    side = [2, 1, 0, 1, 2, 2, 1, 2]
    pool = [w for w, s in enumerate(side) if s]
    assert cn.drawn(side, 3, 5, 0) == [{0, 1, 3}] * 3
    for bits in (1, 2, 4):
        for r, got in enumerate(cn.drawn(side, 8, 5, bits)):
            keys = {w: cn.key(5, r, w, bits) for w in pool}
            assert all(0 <= k < 1 << bits for k in keys.values()) and len(got) == 3
            worst = max((keys[w], w) for w in got)
            assert all((keys[w], w) > worst for w in pool if w not in got)
    assert cn.key(5, 2, 7, 32) == cn.ir.hash32(5, 2, 7) and cn.key(5, 2, 7, 0) == 0
    assert cn.key(1, 0, 0, 4) == 0xE


def test_the_vectorised_keys_and_their_stable_sort_are_the_plain_ones():
    ws = [0, 1, 63, 64, 31243, 2 ** 20 - 1, 2 ** 32 - 1]
    for seed in (0, 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        for r in (0, 1, 999, 4095):
            for bits in (0, 1, 4, 31, 32):
                assert cn.keys_np(seed, r, ws, bits).tolist() == \
                    [cn.key(seed, r, w, bits) for w in ws]
    side = [(w * 5 + 1) % 3 for w in range(300)]
    for bits in (0, 3, 32):
        assert cn.drawn(side, 5, 7, bits, fast=True) == cn.drawn(side, 5, 7, bits)


def test_degenerate_inputs_follow_the_definitions():
    recs = works_of([[(0, 6)], [(0, 6)], [(0, 3)]])
    unit_of = [0] * 6 + [1] * 4
    # every pool work quotes unit 0 (den = 0); nobody quotes unit 1
    units, perms, a_r = cn.contrast(recs, 3, 10, unit_of, 2, [1, 2, 0], min_quoting=1,
                                    permutations=3)
    assert units == [dict(a_works=1, b_works=1, ge=3, adj_ge=3, statistic=0, d=0),
                     dict(a_works=0, b_works=0, ge=3, adj_ge=NONE, statistic=0, d=0)]
    assert [p["max_statistic"] for p in perms] == [0] * 3 and perms[0]["max_unit"] == 0
    # an empty family, an empty side, no records, no units
    units, perms, _ = cn.contrast(recs, 3, 10, unit_of, 2, [1, 2, 0], min_quoting=3, permutations=2)
    assert [u["adj_ge"] for u in units] == [NONE] * 2
    assert perms == [dict(max_statistic=0, a_active=1, max_unit=NONE)] * 2
    units, perms, _ = cn.contrast(recs, 3, 10, unit_of, 2, [0, 2, 2], min_quoting=1, permutations=2)
    assert units[0] == dict(a_works=0, b_works=1, ge=2, adj_ge=2, statistic=0, d=0)
    assert perms == [dict(max_statistic=0, a_active=0, max_unit=0)] * 2
    units, perms, a_r = cn.contrast([], 3, 10, unit_of, 2, [1, 2, 0], permutations=2)
    assert units == [dict(a_works=0, b_works=0, ge=2, adj_ge=NONE, statistic=0, d=0)] * 2
    assert perms == [dict(max_statistic=0, a_active=0, max_unit=NONE)] * 2 and a_r == [[0, 0]] * 2
    assert cn.contrast(recs, 3, 10, [NONE] * 10, 0, [1, 2, 0], permutations=1)[0] == []
    for bad in (dict(min_words=0), dict(min_quoting=0), dict(permutations=0),
                dict(permutations=4097), dict(key_bits=33), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            cn.contrast(recs, 3, 10, unit_of, 2, [1, 2, 0], **bad)
    with pytest.raises(ValueError):
        cn.contrast(recs, 3, 10, unit_of, 2, [1, 3, 0])


# ---- the restatement against theory --------------------------------------------------------

def test_the_relabelled_counts_are_hypergeometric():
    """For a unit with t quoting pool works a_r(u) is hypergeometric(N, t, NA).  Over P = 4096
    permutations its mean lies within 5 standard errors of t NA / N, the variance being
    t (NA / N) (NB / N) (N - t) / (N - 1); GE / P lies within 5 binomial standard deviations of
    the exact two-sided tail.  Both bounds are those of the distributions, not of a run; seed 1."""
    N, NA, P = 200, 75, 4096
    side = [1 if w < NA else 2 for w in range(N)]
    # unit 0: every fifth work and works 1, 2, 3: t = 43, a = 18 against 16.125 expected;
    # unit 1: every third and works 100 .. 105: t = 71, a = 25 against 26.625; unit 2: everybody
    recs = works_of([[(0, 6)] * (w % 5 == 0 or w in (1, 2, 3))
                     + [(10, 6)] * (w % 3 == 0 or 100 <= w <= 105) + [(20, 6)]
                     for w in range(N)])
    unit_of = [0] * 10 + [1] * 10 + [2] * 10
    units, perms, a_r = cn.contrast(recs, N, 30, unit_of, 3, side, min_quoting=5, permutations=P,
                                    seed=1)
    total = math.comb(N, NA)
    for u, t in ((0, 43), (1, 71)):
        assert units[u]["a_works"] + units[u]["b_works"] == t
        mean = sum(a_r[u]) / P
        var = t * (NA / N) * ((N - NA) / N) * (N - t) / (N - 1)
        se = math.sqrt(var / P)
        print("unit", u, "mean", mean, "expected", t * NA / N, "standard error", se)
        assert abs(mean - t * NA / N) <= 5 * se
        d = abs(units[u]["d"])
        tail = sum(math.comb(t, k) * math.comb(N - t, NA - k)
                   for k in range(max(0, NA - (N - t)), min(t, NA) + 1)
                   if abs(k * N - t * NA) >= d) / total
        sd = math.sqrt(tail * (1 - tail) / P)
        print("unit", u, "GE / P", units[u]["ge"] / P, "exact tail", tail, "deviation", sd)
        assert 0 < tail < 1 and abs(units[u]["ge"] / P - tail) <= 5 * sd
    assert all(c == NA for c in a_r[2]) and units[2]["statistic"] == 0
    assert all(p["a_active"] == NA for p in perms)


# ---- the denominators --------------------------------------------------------------------

@pytest.mark.parametrize("root", [1 << 20, (1 << 20) + 1, 1048575, 759250124, 759250125,
                                  (1 << 29) + 12345, 536870911])
def test_isqrt_below_at_and_above_squares_near_2_40_and_2_59(root):
    L = _lib.load()
    for x in (root * root - 1, root * root, root * root + 1):
        assert L.fs_contrast_isqrt(x) == math.isqrt(x) == root - (x < root * root), x
    for x in (0, 1, 2, 3, 4, 2 ** 64 - 1, 2 ** 64 - 2 ** 33, (2 ** 32 - 1) ** 2 - 1):
        assert L.fs_contrast_isqrt(x) == math.isqrt(x), x


def test_a_double_square_root_alone_is_off_by_one_there():
    off = [r for r in (759250124, 759250125, (1 << 29) + 12345, 536870911)
           if int(math.sqrt(float(r * r - 1))) != math.isqrt(r * r - 1)]
    assert off                                       # r^2 - 1 rounds to r^2 as a double
    # den at a t (N - t) that is a square, one less and one more
    assert cn.den(1 << 19, 1 << 20) == 1 << 29                 # 2^38 << 20
    assert cn.den(4, 8) == 4096 and cn.den(3, 8) == math.isqrt(15 << 20) == 3965
    assert cn.den(2, 19) == math.isqrt(34 << 20) == 5970 and cn.den(0, 5) == cn.den(5, 5) == 0
    assert cn.statistic(-3, 2048) == 1536 and cn.statistic(7, 0) == 0


# ---- the sides ---------------------------------------------------------------------------

META = ("FILENAME,TITLE,AUTHOR,SUMMARY,NOTES,PUBLICATION_DATE,LANGUAGE,TAGS\r\n"
        'a.html,,anna,,,2015-12-20,English,"{""Additional Tags"": ""Fluff; Angst"", '
        '""Relationship"": ""Rey/Finn""}"\r\n'
        'b.html,,bob,,,2016-01-02,English,"{""Additional Tags"": ""Fluff""}"\r\n'
        'c.html,,anna,,,2016-03-09,Deutsch,"{""Additional Tags"": ""Angst""}"\r\n'
        'd.html,,dora,,,,English,"{""Relationship"": ""Rey/Finn; Rey & Poe""}"\r\n')
NAMES = ["x/a.txt", "b.txt", "c.txt", "d.txt", "e.txt"]


def both_sides(by, a_keys, b_keys):
    meta = gr.read_meta(META, by)
    got = contrast.sides_of(NAMES, meta, by, a_keys, b_keys)
    want = cn.sides_of(NAMES, meta, by, a_keys, b_keys)
    assert got[0].dtype == np.uint8 and got[0].tolist() == want[0] and got[1] == want[1]
    return want


def test_sides_of():
    # --b absent: B is every work that does not match A, the one without a row included
    assert both_sides("year", ["2016"], []) == ([2, 1, 1, 2, 2], (2, 3, 0, 0))
    # --b present: a work of neither list is out
    assert both_sides("year", ["2016"], ["2015"]) == ([2, 1, 1, 0, 0], (2, 1, 0, 2))
    # a work matching both lists is on neither side
    assert both_sides("tag", ["Additional Tags: Fluff"], ["Additional Tags: Angst"]) == \
        ([0, 1, 2, 0, 0], (1, 1, 1, 2))
    # a work without a metadata row, and one without a date
    assert both_sides("year", ["(no metadata)", "(unknown date)"], []) == \
        ([2, 2, 2, 1, 1], (2, 3, 0, 0))
    # tag:<Category>: the values without the category in front
    assert both_sides("tag:Relationship", ["Rey/Finn"], ["(none)"]) == \
        ([1, 2, 2, 1, 0], (2, 2, 0, 1))
    assert both_sides("author", ["anna"], ["bob", "dora"]) == ([1, 2, 1, 2, 0], (2, 2, 0, 1))
    # an empty side is an error that names it
    meta = gr.read_meta(META, "language")
    for fn in (contrast.sides_of, cn.sides_of):
        with pytest.raises(ValueError, match="side A is empty"):
            fn(NAMES, meta, "language", ["Klingon"], [])
        with pytest.raises(ValueError, match="side B is empty"):
            fn(NAMES, meta, "language", ["English"], ["Klingon"])
    with pytest.raises(ValueError, match="one work"):
        contrast.sides_of(["a.txt", "y/a.html"], meta, "language", ["English"], [])


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["contrast", "runs/m.csv", "meta.csv", "--a", "2016"])
    assert args.func.__name__ == "_contrast"
    assert (args.meta, args.a, args.b, args.by, args.output, args.unit, args.min_words,
            args.max_gap, args.min_works, args.min_quoting, args.permutations, args.seed,
            args.device, args.reader) == \
        ("meta.csv", ["2016"], None, "year", None, "region", 6, 0, 1, 5, 1000, 0, 0, None)
    assert contrast.output_names(args.matches) == (
        "runs/m-contrast.csv", "runs/m-contrast-sides.csv", "runs/m-contrast-permutations.csv")
    assert contrast.output_names("m.csv", "out/x")[2] == "out/x-contrast-permutations.csv"
    args = cli.ao3_parser().parse_args(
        ["contrast", "m.csv", "meta.csv", "--a", "x", "--a", "y z", "--b", "w", "--b", "v",
         "--by", "tag:Relationship", "-o", "p", "--unit", "word", "--min-words", "3",
         "--max-gap", "2", "--min-works", "4", "--min-quoting", "7", "--permutations", "64",
         "--seed", str(2 ** 64 - 1), "--device", "1", "--reader", "python"])
    assert (args.a, args.b, args.by, args.output, args.unit, args.min_words, args.max_gap,
            args.min_works, args.min_quoting, args.permutations, args.seed, args.device,
            args.reader) == (["x", "y z"], ["w", "v"], "tag:Relationship", "p", "word", 3, 2, 4,
                             7, 64, 2 ** 64 - 1, 1, "python")
    for unit in contrast.UNIT:
        assert cli.ao3_parser().parse_args(
            ["contrast", "m", "meta", "--a", "k", "--unit", unit]).unit == unit
    assert contrast.UNIT == ("region", "word", "scene", "character")
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["contrast", "m.csv", "meta.csv", "--a", "k", "--unit", "line"])
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["contrast", "m.csv", "meta.csv"])       # no --a
    assert "contrast" in cli.ao3_parser().format_help()
    assert "contrast" not in cli.full_parser().format_help()
    assert "contrast" in _lib.TIMED
    assert contrast.UNIT_FIELDS == cn.UNIT_FIELDS and contrast.SIDE_FIELDS == cn.SIDE_FIELDS
    assert contrast.PERMUTATION_FIELDS == cn.PERMUTATION_FIELDS
    assert contrast.EVERY_OTHER == cn.EVERY_OTHER


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--max-gap", "-1"],
                                 ["--min-quoting", "0"], ["--permutations", "0"],
                                 ["--permutations", "4097"], ["--seed", "-1"],
                                 ["--seed", str(2 ** 64)], ["--by", "colour"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    meta = tmp_path / "meta.csv"
    meta.write_text(META, encoding="utf-8", newline="")
    with pytest.raises(SystemExit) as e:
        cli.main(["contrast", str(tmp_path / "none.csv"), str(meta), "--a", "2016"] + bad)
    assert str(e.value.code).startswith("ao3.py contrast: error: ")
    assert "\n" not in str(e.value.code)


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_contrast", "fs_contrast_rows", "fs_contrast_times", "fs_contrast_isqrt"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.CONTRAST_MS_NAMES == ("incidence", "selection", "product", "sweeps", "total")
    assert re.search(r"#define FS_CONTRAST_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_CONTRAST_MAX_WORKS \(1u << 20\)", text)
    assert re.search(r"#define FS_CONTRAST_MAX_PERMUTATIONS 4096u", text)
    assert (abi.FS_CONTRAST_MAX_BYTES, abi.FS_CONTRAST_MAX_WORKS,
            abi.FS_CONTRAST_MAX_PERMUTATIONS) == (1 << 30, 1 << 20, 4096)
    # one copy of the hash, in the shared header
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    for unit in ("fs_intervals.hip", "fs_contrast.hip"):
        body = open(os.path.join(src, unit)).read()
        assert "fs_work_hash(" in body and "0xBF58476D1CE4E5B9" not in body
    assert open(os.path.join(src, "fs_hash.h")).read().count("0xBF58476D1CE4E5B9") == 1


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_contrast_unit", "CONTRAST_UNIT_DTYPE", cn.UNIT_KEYS, 32),
    ("fs_contrast_perm", "CONTRAST_PERM_DTYPE", cn.PERM_KEYS, 16)])
def test_dtypes_match_the_header(struct, dtype, keys, size):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for sign, bits, names in re.findall(r"\b(u?)int(32|64)_t\s+([^;]+);", body):
        for n in names.split(","):
            at = (at + int(bits) // 8 - 1) // (int(bits) // 8) * (int(bits) // 8)
            fields.append((n.strip(), at, int(bits) // 8, "u" if sign else "i"))
            at += int(bits) // 8
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize, dt.fields[n][0].kind)
            for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    side = np.zeros(4, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    units = np.ones(2, dtype=abi.CONTRAST_UNIT_DTYPE)
    perms = np.ones(4, dtype=abi.CONTRAST_PERM_DTYPE)
    up, pp = units.ctypes.data_as(C.c_void_p), perms.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_works=1, n_script=4, unit_of=u32, n_units=2, min_words=1, side=side,
             min_quoting=1, permutations=4, key_bits=32, out=up, out_perms=pp, cols=u32):
        return L.fs_contrast(0, cols, cols, cols, n_rows, n_works, n_script, unit_of, n_units,
                             min_words, 0, side, min_quoting, permutations, 0, key_bits, out,
                             out_perms, None)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(n_works=(1 << 20) + 1) == abi.FS_E_UNSUPPORTED
    assert b"1048576" in L.fs_last_error()
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_quoting=0) == abi.FS_E_INVALID
    for permutations in (0, 4097):
        assert call(permutations=permutations) == abi.FS_E_INVALID
    assert call(key_bits=33) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(out_perms=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(side=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["ge"] == 1).all() and (perms["a_active"] == 1).all()       # nothing written
    assert L.fs_contrast_times(None) == abi.FS_E_INVALID
    assert L.fs_contrast_rows(None, None, 0, 0, None, 0, 1, 0, None, 1, 4, 0, 32, None,
                              None) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        contrast.find_contrast(z, z, z, 4, 5, z, 1, [0] * 4)   # a map of 4 entries for 5 words
    with pytest.raises(ValueError):
        contrast.find_contrast(z, z, z, 4, 4, z, 1, [0] * 3)   # 3 side bytes for 4 works
    with pytest.raises(ValueError):
        contrast.find_contrast(z, z, z, 4, 4, z, 1, [0] * 4, seed=1 << 64)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, side, min_words=6,
                max_gap=0, min_quoting=5, permutations=1000, seed=0, key_bits=32, device=0,
                a_counts=False):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    units, perms, a_r = cn.contrast(recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units,
                                    np.asarray(side).tolist(), min_words, max_gap, min_quoting,
                                    permutations, seed, key_bits)
    u = np.zeros(len(units), dtype=abi.CONTRAST_UNIT_DTYPE)
    for k in cn.UNIT_KEYS:
        u[k] = [d[k] for d in units]
    p = np.zeros(len(perms), dtype=abi.CONTRAST_PERM_DTYPE)
    for k in cn.PERM_KEYS:
        p[k] = [d[k] for d in perms]
    counts = np.array(a_r, dtype=np.uint32).reshape(n_units, permutations)
    return (u, p, counts) if a_counts else (u, p)


def oracle_active(work, fan_ix, orig_ix, n_works, min_words=6, max_gap=0, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    return np.array([bool(c) for c in cn.cr.coverage(recs, n_works, min_words, max_gap)])


def test_the_golden_generator_reproduces_its_committed_files():
    made = mcg.build()
    assert set(made) == {mcg.INPUT, mcg.META} | {n for c in mcg.CASES
                                                  for n in mcg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,by,a_keys,b_keys,unit,m,g,k,q,P,seed", mcg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, by, a_keys, b_keys, unit,
                                                      m, g, k, q, P, seed):
    monkeypatch.setattr(contrast, "find_contrast", oracle_find)
    monkeypatch.setattr(contrast, "active_works", oracle_active)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    meta = contrast.read_meta(os.path.join(GOLDEN, mcg.META), by)
    body = contrast.tables(read_matches(os.path.join(GOLDEN, mcg.INPUT)), meta, by, a_keys,
                           b_keys, unit, m, g, k, q, P, seed)
    heads = (contrast.UNIT_FIELDS, contrast.SIDE_FIELDS, contrast.PERMUTATION_FIELDS)
    for name, head, part in zip(mcg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_input_holds_what_its_generator_says():
    made = mcg.build()

    def table(case, kind):
        text = made[mcg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    names = [r[0] for r in csv.reader(io.StringIO(made[mcg.INPUT], newline=""))][1:]
    assert len(set(names)) == mcg.N_WORKS == 48
    tag = table("tag", 0)
    col = {name: k for k, name in enumerate(cn.UNIT_FIELDS)}
    # the planted line: most of A, few of B, reached by no relabelling, alone or among all
    planted = tag[0]
    assert planted[col["TEXT"]] == "i have a bad feeling about"
    assert (planted[col["A_WORKS"]], planted[col["B_WORKS"]]) == ("12", "3")
    assert (planted[col["GE"]], planted[col["ADJ_GE"]]) == ("0", "0")
    assert planted[col["P_PPM"]] == planted[col["ADJ_PPM"]] == "999"
    assert planted[col["DIRECTION"]] == "A" and planted[col["RATIO_PERMILLE"]] == "8000"
    # a line that passes alone at 5 % and not among the family
    alone = [r for r in tag if int(r[col["P_PPM"]]) <= 50000 < int(r[col["ADJ_PPM"]])]
    assert [(r[col["TEXT"]], r[col["P_PPM"]], r[col["ADJ_PPM"]]) for r in alone] == \
        [("do or do not there is", "32967", "119880")]
    assert [int(r[col["ADJ_GE"]]) for r in tag] == sorted(int(r[col["ADJ_GE"]]) for r in tag)
    assert any(r[col["DIRECTION"]] == "=" and r[col["STATISTIC"]] == "0" for r in tag)
    assert table("tag", 1) == [["A", "Alternate Universe", "16", "15", "7"],
                               ["B", "(every other work)", "32", "30", "7"],
                               ["BOTH", "", "0", "0", ""], ["OUT", "", "0", "0", ""]]
    assert len(table("tag", 2)) == 1000
    years = table("years", 1)
    assert years[0][:3] == ["A", "2016; 2017", "23"] and years[1][:3] == ["B", "2014", "12"]
    assert years[3][:3] == ["OUT", "", "13"] and len(table("years", 2)) == 64
    assert [r[col["SCENE"]] for r in table("years", 0)].count("7, later") == 1
    word = table("language", 0)
    assert [r for r in word if r[col["TEXT"]] == "[?]"][0][1:5] == ["182", "182", "", ""]
    assert len(table("language", 2)) == 40
