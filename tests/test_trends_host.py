"""`ao3.py trends` without a GPU: the restated contract (tests/trends_restated.py) on an example
worked by hand and against the distribution it claims, the period numbers and the errors of the
command, the 64-bit bound, the draw, the parser, the C ABI's declarations, and the committed
expected CSVs under the product's table-building code with the oracle standing in for the
device."""

import csv
import ctypes as C
import io
import math
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, companions, trends
from fandom_search_amd.passages import read_matches
from tests import groups_restated as gr
from tests import trends_restated as tr
from tests.golden import make_trends_golden as mtg
from tests.test_companions_host import oracle_quotes, works_of
from tests.test_contrast_host import oracle_active

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF
OUT = 0xFFFF


# ---- an example small enough to check by hand ---------------------------------------------

def test_six_works_three_units_by_hand():
    """Units 0, 1, 2 are the script words 0-9, 10-19, 20-29.  Works 0, 1, 2, 4, 5 are dated
    x = 0, 1, 3, 2, 3; work 3 has no date.  Work 4 has three stray words and is not active.
    N = 5, X = 9."""
    recs = works_of([[(0, 6), (10, 6)], [(0, 6)], [(10, 6)], [(0, 6), (20, 6)], [(20, 3)],
                     [(0, 6), (10, 6), (20, 6)]])
    unit_of = [0] * 10 + [1] * 10 + [2] * 10
    when = [0, 1, 3, OUT, 2, 3]
    units, perms, s_r = tr.trends(recs, 6, 30, unit_of, 3, when, min_quoting=2, permutations=4,
                                  seed=9)
    # unit 0: works 0, 1, 3, 5, of the pool 0, 1, 5: t = 3, s = 4, D = 4 * 5 - 3 * 9 = -7;
    #   den = isqrt(6 << 20) = 2508, Z = 7168 // 2508 = 2
    # unit 1: works 0, 2, 5: t = 3, s = 6, D = 30 - 27 = 3, Z = 3072 // 2508 = 1
    # unit 2: works 3, 5, of the pool 5: t = 1, s = 3, D = 15 - 9 = 6; den = isqrt(4 << 20) = 2048,
    #   Z = 6144 // 2048 = 3; below min_quoting
    assert [(u["quoting"], u["offset_sum"], u["d"], u["statistic"], u["first_x"], u["last_x"])
            for u in units] == [(3, 4, -7, 2, 0, 3), (3, 6, 3, 1, 0, 3), (1, 3, 6, 3, 3, 3)]
    assert [u["adj_ge"] == NONE for u in units] == [False, False, True]
    assert list(units[0]) == tr.UNIT_KEYS and list(perms[0]) == tr.PERM_KEYS
    pool = [0, 1, 2, 4, 5]
    for r in range(4):
        x_r = {w: when[pool[(tr.ir.hash32(9, r, w) * 5) >> 32]] for w in pool}
        assert perms[r]["offset_sum"] == sum(x_r.values())
        assert [s_r[u][r] for u in range(3)] == [x_r[0] + x_r[1] + x_r[5],
                                                 x_r[0] + x_r[2] + x_r[5], x_r[5]]
        zs = [tr.statistic(s_r[u][r] * 5 - 3 * perms[r]["offset_sum"], 2508) for u in (0, 1)]
        assert perms[r]["max_statistic"] == max(zs)
        assert perms[r]["max_unit"] == zs.index(max(zs))
    d_r = [[s_r[u][r] * 5 - units[u]["quoting"] * perms[r]["offset_sum"] for r in range(4)]
           for u in range(3)]
    assert [u["ge"] for u in units] == [sum(abs(d) >= abs(v["d"]) for d in row)
                                        for row, v in zip(d_r, units)]
    assert units[0]["adj_ge"] == sum(p["max_statistic"] >= 2 for p in perms)


def test_degenerate_inputs_follow_the_definitions():
    recs = works_of([[(0, 6)], [(0, 6)], [(0, 3)]])
    unit_of = [0] * 6 + [1] * 4
    # every pool work quotes unit 0 (t = N: outside the family); nobody quotes unit 1
    units, perms, s_r = tr.trends(recs, 3, 10, unit_of, 2, [4, 7, OUT], min_quoting=1,
                                  permutations=3)
    assert units == [dict(quoting=2, ge=3, adj_ge=NONE, first_x=4, last_x=7, offset_sum=11,
                          statistic=0, d=0),
                     dict(quoting=0, ge=3, adj_ge=NONE, first_x=NONE, last_x=NONE, offset_sum=0,
                          statistic=0, d=0)]
    assert all(p["max_statistic"] == 0 and p["max_unit"] == NONE for p in perms)
    assert all(s_r[0][r] == perms[r]["offset_sum"] for r in range(3))
    # an empty pool, no records, no units
    units, perms, _ = tr.trends(recs, 3, 10, unit_of, 2, [OUT] * 3, permutations=2)
    assert perms == [dict(max_statistic=0, offset_sum=0, max_unit=NONE)] * 2
    assert [u["quoting"] for u in units] == [0, 0]
    units, perms, s_r = tr.trends([], 3, 10, unit_of, 2, [1, 2, OUT], permutations=2)
    assert [u["ge"] for u in units] == [2, 2] and s_r == [[0, 0]] * 2
    assert all(p["offset_sum"] in (2, 3, 4) for p in perms)
    assert tr.trends(recs, 3, 10, [NONE] * 10, 0, [1, 2, OUT], permutations=1)[0] == []
    for bad in (dict(min_words=0), dict(min_quoting=0), dict(permutations=0),
                dict(permutations=4097), dict(seed=2 ** 64)):
        with pytest.raises(ValueError):
            tr.trends(recs, 3, 10, unit_of, 2, [1, 2, OUT], **bad)
    with pytest.raises(ValueError):
        tr.trends(recs, 3, 10, unit_of, 2, [1, 1024, OUT])


# ---- the draw and the distribution -------------------------------------------------------

def test_the_draw_is_uniform_over_the_pool():
    """v = (h * N) >> 32 over 48 000 draws into N = 48 positions: Pearson's statistic has 47
    degrees of freedom, mean 47 and variance 94; it lies within five standard deviations."""
    n, reps, works = 48, 100, 10
    hits = [0] * n
    for r in range(reps):
        for w in range(works * n):
            v = tr.draw(3, r, w, n)
            assert 0 <= v < n
            hits[v] += 1
    expected = reps * works
    chi2 = sum((h - expected) ** 2 for h in hits) / expected
    print("chi2", chi2, "of 47 +- ", math.sqrt(94))
    assert abs(chi2 - 47) <= 5 * math.sqrt(94)
    big = 1 << 20
    assert max(tr.draw(0, r, w, big) for r in range(4) for w in range(5000)) < big
    assert (0xFFFFFFFF * big) >> 32 == big - 1               # the largest hash stays inside


def test_the_vectorised_draw_is_the_plain_one():
    when = [(w * 37) % 1024 if w % 4 else OUT for w in range(300)]
    for seed in (0, 5, 2 ** 64 - 1):
        assert tr.redated(when, 5, seed, fast=True) == tr.redated(when, 5, seed)
    assert tr.redated([OUT] * 4, 2, 0, fast=True) == [[0] * 4] * 2


def test_the_redated_shifts_have_the_mean_and_the_variance_of_the_draw():
    """D_r = sum over the pool of c(w) x_r(w), c = N - t for the t quoting works and -t for the
    others, the x_r(w) independent draws from the pool's offsets with variance sigma^2.  The c
    sum to 0, so E D_r = 0; Var D_r = sigma^2 sum c^2 = sigma^2 N t (N - t).  Over 4096
    re-datings the mean of D_r lies within five standard errors of 0, and the mean of D_r^2
    within five of the variance, the variance of D_r^2 being 2 V^2 + kappa4 sum c^4 with kappa4
    the fourth cumulant of the offsets.  The bounds are those of the distribution; seed 1."""
    N, P = 200, 4096
    when = [(w * 53) % 240 for w in range(N)]
    recs = works_of([[(0, 6)] * (w % 5 == 0 or w in (1, 2, 3)) + [(10, 6)] for w in range(N)])
    unit_of = [0] * 10 + [1] * 10
    units, perms, s_r = tr.trends(recs, N, 20, unit_of, 2, when, permutations=P, seed=1)
    t = units[0]["quoting"]
    assert t == 43 and units[1]["quoting"] == N and units[1]["adj_ge"] == NONE
    mu = sum(when) / N
    var_x = sum((x - mu) ** 2 for x in when) / N
    m4 = sum((x - mu) ** 4 for x in when) / N
    V = var_x * N * t * (N - t)
    d_r = [s_r[0][r] * N - t * perms[r]["offset_sum"] for r in range(P)]
    mean, mean_sq = sum(d_r) / P, sum(d * d for d in d_r) / P
    se = math.sqrt(V / P)
    c4 = t * (N - t) ** 4 + (N - t) * t ** 4
    se_sq = math.sqrt((2 * V * V + (m4 - 3 * var_x ** 2) * c4) / P)
    print("mean", mean, "standard error", se, "mean square", mean_sq, "variance", V,
          "standard error", se_sq)
    assert abs(mean) <= 5 * se
    assert abs(mean_sq - V) <= 5 * se_sq
    assert all(s_r[1][r] == perms[r]["offset_sum"] for r in range(P))    # everybody: X_r itself


# ---- 64 bits -------------------------------------------------------------------------------

def test_every_intermediate_fits_64_bits_at_the_bounds():
    L = _lib.load()
    n, x = 1 << 20, 1023
    assert n == abi.FS_TRENDS_MAX_WORKS and x == abi.FS_TRENDS_MAX_SPAN - 1
    t = n // 2
    # the quoting half at 1023 and the rest at 0, and the other way round
    for s, big_x in ((t * x, t * x), (0, t * x), (t * x, n * x)):
        d = s * n - t * big_x
        assert abs(d) <= 1 << 50 and s * n < 1 << 63 and t * big_x < 1 << 63
        assert abs(d) << 10 < 1 << 63
    inside = (t * (n - t)) << 20
    assert t * (n - t) == 1 << 38 and inside == 1 << 58
    assert L.fs_contrast_isqrt(inside) == math.isqrt(inside) == tr.den(t, n) == 1 << 29
    d = t * x * n - t * t * x                                # the largest |D|: 1023 * 2^38
    assert tr.statistic(d, tr.den(t, n)) == (d << 10) >> 29 == 1023 << 19
    assert ((C.c_uint64(d << 10).value // L.fs_contrast_isqrt(inside))
            == tr.statistic(-d, tr.den(t, n)))
    # a plane's sum stays inside 32 bits, and so does their recombination
    assert n * 127 < 1 << 27 and n * 7 < 1 << 23 and n * 127 + 128 * n * 7 == n * x < 1 << 30
    for t, nn in ((1, 2), (3, 8), (2, 19), (n - 1, n)):
        assert L.fs_contrast_isqrt((t * (nn - t)) << 20) == tr.den(t, nn)
    assert tr.den(0, 5) == tr.den(5, 5) == 0 and tr.statistic(7, 0) == 0


# ---- the periods ---------------------------------------------------------------------------

META = ("FILENAME,TITLE,AUTHOR,SUMMARY,NOTES,PUBLICATION_DATE,LANGUAGE,TAGS\r\n"
        'a.html,,anna,,,2015-12-20,English,"{}"\r\n'
        'b.html,,bob,,,2016-01-02,English,"{}"\r\n'
        'c.html,,anna,,,2018-03-09,Deutsch,"{}"\r\n'
        'd.html,,dora,,,,English,"{}"\r\n')
NAMES = ["x/a.txt", "b.txt", "c.txt", "d.txt", "e.txt"]


def test_period_numbers_and_offsets():
    assert trends.number_of("2016") == tr.number_of("2016") == 2016
    assert trends.number_of("2016-01") == tr.number_of("2016-01") == 2016 * 12
    assert trends.number_of("2015-12") == 2016 * 12 - 1
    for by, number, label in (("year", 2016, "2016"), ("month", 24192, "2016-01"),
                              ("month", 24191, "2015-12"), ("year", 987, "0987")):
        assert trends.label_of(number, by) == tr.label_of(number, by) == label
        assert trends.number_of(label) == number
    for by, want, base in (("year", [0, 1, 3, OUT, OUT], 2015),
                           ("month", [0, 1, 27, OUT, OUT], 2015 * 12 + 11)):
        meta = gr.read_meta(META, by)
        when, got_base, keys = trends.periods_of(NAMES, meta, by)
        assert when.dtype == np.uint16 and when.tolist() == want and got_base == base
        assert (when.tolist(), got_base, keys) == tr.periods_of(NAMES, meta, by)
        assert keys[3:] == ["(unknown date)", "(no metadata)"]
    with pytest.raises(ValueError, match="one work"):
        trends.periods_of(["a.txt", "y/a.html"], gr.read_meta(META, "year"), "year")


def meta_of(dates):
    rows = ["FILENAME,TITLE,AUTHOR,SUMMARY,NOTES,PUBLICATION_DATE,LANGUAGE,TAGS"]
    rows += ['w%02d.html,,,,,%s,English,"{}"' % (i, d) for i, d in enumerate(dates)]
    return "\r\n".join(rows) + "\r\n"


def test_the_span_at_and_above_its_bound():
    names = ["w00.txt", "w01.txt", "w02.txt"]
    meta = gr.read_meta(meta_of(["1900-01-01", "1985-04-30", "1950-06-15"]), "month")
    when, base, _ = trends.periods_of(names, meta, "month")
    assert when.tolist() == [0, 1023, 605] and base == 1900 * 12
    meta = gr.read_meta(meta_of(["1900-01-01", "1985-05-01", "1950-06-15"]), "month")
    for fn in (trends.periods_of, tr.periods_of):
        with pytest.raises(ValueError, match="span"):
            fn(names, meta, "month")
    meta = gr.read_meta(meta_of(["0976-01-01", "2000-05-01", ""]), "year")
    with pytest.raises(ValueError, match="from 0976 to 2000 span 1024 periods, more than 1023"):
        trends.periods_of(names, meta, "year")


def command_error(tmp_path, meta_text, more=()):
    meta = tmp_path / "meta.csv"
    meta.write_text(meta_text, encoding="utf-8", newline="")
    with pytest.raises(SystemExit) as e:
        cli.main(["trends", os.path.join(GOLDEN, mtg.INPUT), str(meta), "--reader", "python"]
                 + list(more))
    text = str(e.value.code)
    assert text.startswith("ao3.py trends: error: ") and "\n" not in text
    return text[len("ao3.py trends: error: "):]


def test_pools_the_command_refuses_with_one_line(tmp_path):
    """The pool is decided before a passage is looked for: no GPU is touched."""
    assert command_error(tmp_path, meta_of(["2015-%02d-01" % (1 + i % 12) for i in range(48)])) \
        == "every dated work of the match file is of the year 2015: a trend needs two periods"
    assert command_error(tmp_path, meta_of([""] * 48)) \
        == "the pool is empty: no work of the match file has a publication date"
    assert command_error(tmp_path, meta_of([])) \
        == "the pool is empty: no work of the match file has a publication date"
    far = ["1900-01-01", "1985-05-01"] + ["1950-06-15"] * 46
    assert command_error(tmp_path, meta_of(far), ["--by", "month"]) \
        == "the months from 1900-01 to 1985-05 span 1024 periods, more than 1023"
    for by in ("author", "language", "tag", "tag:Rating", "decade"):
        assert command_error(tmp_path, meta_of(far), ["--by", by]) \
            == "--by takes year or month, not %r" % by
    two = "FILENAME,PUBLICATION_DATE\r\nw00.html,2015-01-01\r\nw00.txt,2016-01-01\r\n"
    assert "two rows for the work 'w00'" in command_error(tmp_path, two)       # (groups' own)
    assert "has no PUBLICATION_DATE column" in command_error(tmp_path, "FILENAME\r\nw00\r\n")


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["trends", "runs/m.csv", "meta.csv"])
    assert args.func.__name__ == "_trends"
    assert (args.meta, args.by, args.output, args.unit, args.min_words, args.max_gap,
            args.min_works, args.min_quoting, args.permutations, args.seed, args.device,
            args.reader) == ("meta.csv", "year", None, "region", 6, 0, 1, 5, 1000, 0, 0, None)
    assert trends.output_names(args.matches) == (
        "runs/m-trends.csv", "runs/m-trends-periods.csv", "runs/m-trends-permutations.csv")
    assert trends.output_names("m.csv", "out/x")[2] == "out/x-trends-permutations.csv"
    args = cli.ao3_parser().parse_args(
        ["trends", "m.csv", "meta.csv", "--by", "month", "-o", "p", "--unit", "word",
         "--min-words", "3", "--max-gap", "2", "--min-works", "4", "--min-quoting", "7",
         "--permutations", "64", "--seed", str(2 ** 64 - 1), "--device", "1", "--reader",
         "python"])
    assert (args.by, args.output, args.unit, args.min_words, args.max_gap, args.min_works,
            args.min_quoting, args.permutations, args.seed, args.device, args.reader) == \
        ("month", "p", "word", 3, 2, 4, 7, 64, 2 ** 64 - 1, 1, "python")
    for unit in trends.UNIT:
        assert cli.ao3_parser().parse_args(["trends", "m", "meta", "--unit", unit]).unit == unit
    assert trends.UNIT == ("region", "word", "scene", "character")
    assert trends.BY == ("year", "month")
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["trends", "m.csv", "meta.csv", "--unit", "line"])
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["trends", "m.csv"])                 # no metadata csv
    assert "trends" in cli.ao3_parser().format_help()
    assert "trends" not in cli.full_parser().format_help()
    assert "trends" in _lib.TIMED
    assert trends.UNIT_FIELDS == tr.UNIT_FIELDS and trends.PERIOD_FIELDS == tr.PERIOD_FIELDS
    assert trends.PERMUTATION_FIELDS == tr.PERMUTATION_FIELDS


@pytest.mark.parametrize("bad,message", [
    (["--min-words", "0"], "--min-words, --min-works and --min-quoting must be at least 1, "
                           "--max-gap at least 0"),
    (["--min-works", "0"], "--min-words, --min-works and --min-quoting must be at least 1, "
                           "--max-gap at least 0"),
    (["--min-quoting", "0"], "--min-words, --min-works and --min-quoting must be at least 1, "
                             "--max-gap at least 0"),
    (["--max-gap", "-1"], "--min-words, --min-works and --min-quoting must be at least 1, "
                          "--max-gap at least 0"),
    (["--permutations", "0"], "--permutations must be from 1 to 4096"),
    (["--permutations", "4097"], "--permutations must be from 1 to 4096"),
    (["--seed", "-1"], "--seed must be from 0 to 2^64 - 1"),
    (["--seed", str(2 ** 64)], "--seed must be from 0 to 2^64 - 1"),
    (["--by", "colour"], "--by takes year or month, not 'colour'")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    meta = tmp_path / "meta.csv"
    meta.write_text(META, encoding="utf-8", newline="")
    with pytest.raises(SystemExit) as e:
        cli.main(["trends", str(tmp_path / "none.csv"), str(meta)] + bad)
    assert str(e.value.code) == "ao3.py trends: error: " + message


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_trends", "fs_trends_rows", "fs_trends_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.TRENDS_MS_NAMES == ("pool", "labels", "product", "sweeps", "total")
    assert re.search(r"#define FS_TRENDS_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_TRENDS_MAX_WORKS \(1u << 20\)", text)
    assert re.search(r"#define FS_TRENDS_MAX_SPAN 1024u", text)
    assert re.search(r"#define FS_TRENDS_MAX_PERMUTATIONS 4096u", text)
    assert (abi.FS_TRENDS_MAX_BYTES, abi.FS_TRENDS_MAX_WORKS, abi.FS_TRENDS_MAX_SPAN,
            abi.FS_TRENDS_MAX_PERMUTATIONS, abi.TRENDS_OUT) == (1 << 30, 1 << 20, 1024, 4096, OUT)
    # the hash stays in the shared header, and the product is the matrix instruction
    src = os.path.join(ROOT, "fandom_search_amd", "csrc")
    body = open(os.path.join(src, "fs_trends.hip")).read()
    assert "fs_work_hash(" in body and "0xBF58476D1CE4E5B9" not in body
    assert "__builtin_amdgcn_mfma_i32_16x16x64_i8" in body and "asm" not in body
    assert "fs_trends.hip" in open(os.path.join(src, "Makefile")).read()


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_trends_unit", "TRENDS_UNIT_DTYPE", tr.UNIT_KEYS[:5] + ["reserved"] + tr.UNIT_KEYS[5:], 48),
    ("fs_trends_perm", "TRENDS_PERM_DTYPE", tr.PERM_KEYS, 16)])
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
    when = np.zeros(4, dtype=np.uint16).ctypes.data_as(C.c_void_p)
    units = np.ones(2, dtype=abi.TRENDS_UNIT_DTYPE)
    perms = np.ones(4, dtype=abi.TRENDS_PERM_DTYPE)
    up, pp = units.ctypes.data_as(C.c_void_p), perms.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_works=1, n_script=4, unit_of=u32, n_units=2, min_words=1, when=when,
             min_quoting=1, permutations=4, out=up, out_perms=pp, cols=u32):
        return L.fs_trends(0, cols, cols, cols, n_rows, n_works, n_script, unit_of, n_units,
                           min_words, 0, when, min_quoting, permutations, 0, out, out_perms, None)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(n_works=(1 << 20) + 1) == abi.FS_E_UNSUPPORTED
    assert b"1048576" in L.fs_last_error()
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_quoting=0) == abi.FS_E_INVALID
    for permutations in (0, 4097):
        assert call(permutations=permutations) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(out_perms=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(when=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["ge"] == 1).all() and (perms["offset_sum"] == 1).all()     # nothing written
    assert L.fs_trends_times(None) == abi.FS_E_INVALID
    assert L.fs_trends_rows(None, None, 0, 0, None, 0, 1, 0, None, 1, 4, 0, None,
                            None) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        trends.find_trends(z, z, z, 4, 5, z, 1, [0] * 4)       # a map of 4 entries for 5 words
    with pytest.raises(ValueError):
        trends.find_trends(z, z, z, 4, 4, z, 1, [0] * 3)       # 3 offsets for 4 works
    with pytest.raises(ValueError):
        trends.find_trends(z, z, z, 4, 4, z, 1, [0] * 4, seed=1 << 64)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, when, min_words=6,
                max_gap=0, min_quoting=5, permutations=1000, seed=0, device=0, sums=False):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    units, perms, s_r = tr.trends(recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units,
                                  np.asarray(when).tolist(), min_words, max_gap, min_quoting,
                                  permutations, seed)
    u = np.zeros(len(units), dtype=abi.TRENDS_UNIT_DTYPE)
    for k in tr.UNIT_KEYS:
        u[k] = [d[k] for d in units]
    p = np.zeros(len(perms), dtype=abi.TRENDS_PERM_DTYPE)
    for k in tr.PERM_KEYS:
        p[k] = [d[k] for d in perms]
    table = np.array(s_r, dtype=np.uint32).reshape(n_units, permutations)
    return (u, p, table) if sums else (u, p)


def test_the_golden_generator_reproduces_its_committed_files():
    made = mtg.build()
    assert set(made) == {n for c in mtg.CASES for n in mtg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,by,unit,m,g,k,q,P,seed", mtg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, by, unit, m, g, k, q, P,
                                                      seed):
    monkeypatch.setattr(trends, "find_trends", oracle_find)
    monkeypatch.setattr(trends, "active_works", oracle_active)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    meta = trends.read_meta(os.path.join(GOLDEN, mtg.META), by)
    body = trends.tables(read_matches(os.path.join(GOLDEN, mtg.INPUT)), meta, by, unit, m, g, k,
                         q, P, seed)
    heads = (trends.UNIT_FIELDS, trends.PERIOD_FIELDS, trends.PERMUTATION_FIELDS)
    for name, head, part in zip(mtg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_goldens_hold_what_the_contract_says():
    made = mtg.build()

    def table(case, kind):
        text = made[mtg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    col = {name: k for k, name in enumerate(tr.UNIT_FIELDS)}
    year = table("year", 0)
    assert [int(r[col["ADJ_GE"]]) for r in year] == sorted(int(r[col["ADJ_GE"]]) for r in year)
    for r in year:
        t, mean, pool = (int(r[col[k]]) for k in ("QUOTING_WORKS", "MEAN_PERIOD_MILLI",
                                                  "POOL_MEAN_PERIOD_MILLI"))
        assert t >= 5 and pool == 2014000 + (11 + 24 + 33) * 1000 // 46
        want = "later" if mean > pool else "earlier"
        assert r[col["DIRECTION"]] in (want, "=") and 2014000 <= mean <= 2017000
        assert int(r[col["P_PPM"]]) == (int(r[col["GE"]]) + 1) * 1000000 // 1001
    assert table("year", 1) == [["2014", "0", "12", "12"], ["2015", "1", "11", "9"],
                                ["2016", "2", "12", "12"], ["2017", "3", "11", "10"],
                                ["(unknown date)", "", "1", "1"], ["(no metadata)", "", "1", "1"]]
    assert len(table("year", 2)) == 1000 and len(table("month_scene", 2)) == 64
    months = table("month_scene", 1)
    assert months[0][:2] == ["2014-01", "0"] and months[-3][:2] == ["2017-11", "46"]
    assert len(months) == 47 + 2 and any(r[2] == "0" for r in months)    # empty periods are rows
    assert sum(int(r[2]) for r in months) == 48
    assert [r[col["SCENE"]] for r in table("month_scene", 0)].count("7, later") == 1
    word = table("word_gap1", 0)
    assert [r for r in word if r[col["TEXT"]] == "[?]"][0][1:5] == ["182", "182", "", ""]
    assert len(set(r[1] for r in table("word_gap1", 2))) > 5             # X_r varies
