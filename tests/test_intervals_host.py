"""`ao3.py intervals` without a GPU: the Poisson table, the hash and the multiplicities of the
restated contract (tests/intervals_restated.py), its order statistics and neighbours worked by
hand, the parser, the C ABI's declarations, and the committed expected CSVs under the product's
table-building code with the oracle standing in for the device."""

import csv
import ctypes as C
import decimal
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, companions, intervals
from fandom_search_amd.passages import read_matches
from tests import companions_restated as cr
from tests import intervals_restated as ir
from tests.golden import make_intervals_golden as mig
from tests.test_companions_host import oracle_quotes, works_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


# ---- the multiplicities ------------------------------------------------------------------

def test_the_poisson_table_is_the_distribution_function_at_sixty_digits_and_more():
    for digits in (60, 80, 120):
        assert ir.poisson_table(digits) == ir.T
    # and written out once more, without the restatement's loop
    decimal.getcontext().prec = 70
    e_inv = decimal.Decimal(-1).exp()
    cdf, fact = decimal.Decimal(0), 1
    for k, t in enumerate(ir.T):
        fact *= max(1, k)
        cdf += e_inv / fact
        assert int(cdf * 2 ** 32) == t, k
    assert len(ir.T) == 13 and ir.T[12] == 2 ** 32 - 1 and list(ir.T) == sorted(set(ir.T))


def test_hash_known_answers():
    # z = 0 stays 0 through every xor-shift and product
    assert ir.hash32(0, 0, 0) == 0 and ir.mult(0, 0, 0) == 0
    # seed 1, b = w = 0: z starts at the golden gamma, the first output of splitmix64 from
    # state 0, 0xE220A8397B1DCDAF in every published table of that generator
    assert ir.hash32(1, 0, 0) == 0xE220A839
    # w = 1: z = 1, so the first product is the multiplier itself
    z = 0xBF58476D1CE4E5B9
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert ir.hash32(0, 0, 1) == (z ^ (z >> 31)) >> 32 == 0x5692161D
    # b sits above bit 32, w below: the largest of both, and the largest seed (-gamma mod 2^64)
    assert ir.hash32(0, 4095, 0xFFFFFFFF) == 0x3C02895C
    assert ir.hash32(2 ** 64 - 1, 4095, 0xFFFFFFFF) == 0x91144CFF
    assert ir.hash32(0, 1, 0) != ir.hash32(0, 0, 1)
    # a multiplicity counts the table entries at or below h
    assert [ir.mult(1, 0, 0), ir.mult(0, 0, 1)] == [2, 0]
    assert 0xE220A839 >= ir.T[1] and 0xE220A839 < ir.T[2] and 0x5692161D < ir.T[0]


def test_the_vectorised_multiplicity_is_the_plain_one():
    bs, ws = [0, 1, 15, 16, 999, 4095], [0, 1, 63, 64, 31243, 2 ** 28, 2 ** 32 - 1]
    for seed in (0, 1, 7, 2 ** 63 + 12345, 2 ** 64 - 1):
        got = ir.mult_np(seed, bs, ws)
        assert got.dtype == np.uint8 and got.shape == (len(bs), len(ws))
        assert got.tolist() == [[ir.mult(seed, b, w) for w in ws] for b in bs]


def test_mean_multiplicity_over_a_million_pairs():
    """Poisson(1) has variance 1: the standard error of the mean of 10^6 draws is 0.001, so
    1 +- 0.01 is ten of them; a table shifted by one row or a wrong shift in the hash moves the
    mean by 0.3 and more."""
    m = ir.mult_np(0, range(1000), range(1000)).astype(np.int64)
    mean = m.sum() / m.size
    print("mean multiplicity", mean, "largest", m.max())
    assert abs(mean - 1) <= 0.01
    share = np.bincount(m.ravel(), minlength=4)[:4] / m.size     # e^-1, e^-1, e^-1 / 2, e^-1 / 6
    assert np.abs(share - np.array([0.3679, 0.3679, 0.1839, 0.0613])).max() < 0.003


# ---- order statistics and neighbours -----------------------------------------------------

@pytest.mark.parametrize("B,level,t", [(1, 50, 0), (1, 95, 0), (1, 99, 0), (2, 50, 0), (2, 95, 0),
                                       (2, 99, 0), (39, 50, 9), (39, 95, 0), (39, 99, 0),
                                       (40, 50, 10), (40, 95, 1), (40, 99, 0), (41, 50, 10),
                                       (41, 95, 1), (41, 99, 0)])
def test_order_statistics(B, level, t):
    assert ir.cut(B, level) == t
    values = [(k * 7919) % 101 for k in range(B)]              # no order to begin with
    low, med, high = ir.order_stats(values, level)
    s = sorted(values)
    assert (low, med, high) == (s[t], s[(B - 1) // 2], s[B - 1 - t])
    assert low <= med <= high
    assert ir.order_stats(list(range(B)), level) == (t, (B - 1) // 2, B - 1 - t)


def test_next_under_ties_is_the_lower_unit_first():
    assert ir.observed_order([3, 5, 3, 5, 0]) == [1, 3, 0, 2, 4]
    # three works; unit 0 by works 0 and 1, units 1 and 2 by all three, unit 3 by nobody
    recs = works_of([[(0, 6), (10, 6), (20, 6)], [(0, 6), (10, 6), (20, 6)], [(10, 6), (20, 6)]])
    unit_of = [0] * 10 + [1] * 10 + [2] * 10 + [3] * 5
    units, reps = ir.intervals(recs, 3, 35, unit_of, 4, replicates=16, seed=3, level=90)
    assert [u["works"] for u in units] == [2, 3, 3, 0]
    assert [u["rank"] for u in units] == [3, 1, 1, 4]
    assert [u["next"] for u in units] == [3, 2, 0, NONE]
    assert (units[1]["ahead"], units[1]["tied"], units[1]["behind"]) == (0, 16, 0)
    assert all(u["ahead"] + u["tied"] + u["behind"] == 16 for u in units[:3])
    assert (units[3]["ahead"], units[3]["tied"], units[3]["behind"]) == (0, 0, 0)
    assert units[0]["behind"] == 0                             # against a unit nobody quotes
    assert list(units[0]) == ir.UNIT_KEYS and list(reps[0]) == ir.REPLICATE_KEYS
    # every figure of replicate b from the multiplicities of the three works
    for b, r in enumerate(reps):
        m = [ir.mult(3, b, w) for w in range(3)]
        assert (r["resampled_works"], r["resampled_active"]) == (sum(m), sum(m))
        assert r["units_quoted"] == (m[0] + m[1] > 0) + 2 * (sum(m) > 0)
    total = sum(ir.mult(3, b, w) for b in range(16) for w in (0, 1))
    assert units[0]["mean_milli"] == total * 1000 // 16
    assert units[0]["ppm"] == 2 * 1000000 // 3


def test_an_inactive_work_is_resampled_and_quotes_nothing():
    recs = works_of([[(0, 6)], [(0, 3)], [(1, 6)]])            # work 1: three stray words
    units, reps = ir.intervals(recs, 3, 10, [0] * 10, 1, replicates=33, seed=5)
    assert units[0]["works"] == 2 and units[0]["ppm"] == 666666
    assert any(r["resampled_works"] != r["resampled_active"] for r in reps)
    for b, r in enumerate(reps):
        assert r["resampled_works"] - r["resampled_active"] == ir.mult(5, b, 1)
    none, reps0 = ir.intervals([], 0, 0, [], 0, replicates=2)
    assert none == [] and reps0 == [dict(resampled_works=0, resampled_active=0, units_quoted=0)] * 2
    for bad in (dict(min_words=0), dict(replicates=0), dict(replicates=4097), dict(level=49),
                dict(level=100), dict(seed=2 ** 64), dict(seed=-1)):
        with pytest.raises(ValueError):
            ir.intervals(recs, 3, 10, [0] * 10, 1, **bad)
    assert ir.intervals(recs, 3, 10, [0] * 10, 1, replicates=9, fast=True) == \
        ir.intervals(recs, 3, 10, [0] * 10, 1, replicates=9)


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["intervals", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_intervals"
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.replicates,
            args.seed, args.level, args.device, args.reader) == \
        (None, "region", 6, 0, 1, 1000, 0, 95, 0, None)
    assert intervals.output_names(args.matches) == (
        "runs/match-6gram-20240101-intervals.csv",
        "runs/match-6gram-20240101-intervals-replicates.csv")
    assert intervals.output_names("m.csv", "out/x")[1] == "out/x-intervals-replicates.csv"
    args = cli.ao3_parser().parse_args(
        ["intervals", "m.csv", "-o", "p", "--by", "word", "--min-words", "3", "--max-gap", "2",
         "--min-works", "4", "--replicates", "64", "--seed", str(2 ** 64 - 1), "--level", "90",
         "--device", "1", "--reader", "python"])
    assert (args.output, args.by, args.min_words, args.max_gap, args.min_works, args.replicates,
            args.seed, args.level, args.device, args.reader) == \
        ("p", "word", 3, 2, 4, 64, 2 ** 64 - 1, 90, 1, "python")
    for by in ("scene", "character", "region"):
        assert cli.ao3_parser().parse_args(["intervals", "m", "--by", by]).by == by
    assert intervals.UNIT_FIELDS == ir.UNIT_FIELDS
    assert intervals.REPLICATE_FIELDS == ir.REPLICATE_FIELDS
    assert "intervals" in cli.ao3_parser().format_help()
    with pytest.raises(SystemExit):
        cli.ao3_parser().parse_args(["intervals", "m.csv", "--by", "line"])


@pytest.mark.parametrize("bad", [["--min-words", "0"], ["--min-works", "0"], ["--max-gap", "-1"],
                                 ["--replicates", "0"], ["--replicates", "4097"],
                                 ["--level", "49"], ["--level", "100"], ["--seed", "-1"],
                                 ["--seed", str(2 ** 64)]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["intervals", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py intervals: error: ")
    assert "\n" not in str(e.value.code)


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_intervals", "fs_intervals_rows", "fs_intervals_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "intervals" in _lib.TIMED
    assert abi.INTERVALS_MS_NAMES == ("incidence", "multiplicities", "product", "statistics",
                                      "neighbours", "total")
    assert re.search(r"#define FS_INTERVALS_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_INTERVALS_MAX_REPLICATES 4096u", text)
    assert abi.FS_INTERVALS_MAX_BYTES == 1 << 30 and abi.FS_INTERVALS_MAX_REPLICATES == 4096
    for t in ir.T:                                             # the table, in the header's words
        assert str(t) in text
    src = open(os.path.join(ROOT, "fandom_search_amd", "csrc", "fs_intervals.hip")).read()
    for t in ir.T:
        assert "%du" % t in src


@pytest.mark.parametrize("struct,dtype,keys,size", [
    ("fs_interval_unit", "INTERVAL_UNIT_DTYPE",
     ir.UNIT_KEYS[:-1] + ["reserved", "mean_milli"], 64),
    ("fs_interval_replicate", "INTERVAL_REPLICATE_DTYPE", ir.REPLICATE_KEYS + ["reserved"], 16)])
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
    assert dt.itemsize == size == at
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    units = np.ones(2, dtype=abi.INTERVAL_UNIT_DTYPE)
    reps = np.ones(4, dtype=abi.INTERVAL_REPLICATE_DTYPE)
    up, rp = units.ctypes.data_as(C.c_void_p), reps.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_works=1, n_script=4, unit_of=u32, n_units=2, min_words=1, replicates=4,
             level=95, out=up, out_reps=rp, cols=u32):
        return L.fs_intervals(0, cols, cols, cols, n_rows, n_works, n_script, unit_of, n_units,
                              min_words, 0, replicates, 0, level, out, out_reps)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(n_works=(1 << 28) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    for replicates in (0, 4097):
        assert call(replicates=replicates) == abi.FS_E_INVALID
    for level in (49, 100):
        assert call(level=level) == abi.FS_E_INVALID
    assert call(out=None) == abi.FS_E_INVALID
    assert call(out_reps=None) == abi.FS_E_INVALID
    assert call(unit_of=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (units["works"] == 1).all() and (reps["units_quoted"] == 1).all()   # nothing written
    assert L.fs_intervals_times(None) == abi.FS_E_INVALID
    assert L.fs_intervals_rows(None, None, 0, 0, None, 0, 1, 0, 4, 0, 95, None,
                               None) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        intervals.find_intervals(z, z, z, 1, 5, z, 1)          # a map of 4 entries for 5 words
    with pytest.raises(ValueError):
        intervals.find_intervals(z, z, z, 1, 4, z, 1, seed=1 << 64)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, replicates=1000, seed=0, level=95, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    units, reps = ir.intervals(recs, n_works, n_script, np.asarray(unit_of).tolist(), n_units,
                               min_words, max_gap, replicates, seed, level)
    u = np.zeros(len(units), dtype=abi.INTERVAL_UNIT_DTYPE)
    for k in ir.UNIT_KEYS:
        u[k] = [d[k] for d in units]
    r = np.zeros(len(reps), dtype=abi.INTERVAL_REPLICATE_DTYPE)
    for k in ir.REPLICATE_KEYS:
        r[k] = [d[k] for d in reps]
    return u, r


def test_the_golden_generator_reproduces_its_committed_files():
    made = mig.build()
    assert set(made) == {mig.INPUT} | {n for c in mig.CASES for n in mig.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,by,min_words,max_gap,min_works,replicates,seed,level", mig.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, by, min_words, max_gap,
                                                      min_works, replicates, seed, level):
    monkeypatch.setattr(intervals, "find_intervals", oracle_find)
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    body = intervals.tables(read_matches(os.path.join(GOLDEN, mig.INPUT)), by, min_words,
                            max_gap, min_works, replicates, seed, level)
    for name, head, part in zip(mig.golden_names(case),
                                (intervals.UNIT_FIELDS, intervals.REPLICATE_FIELDS), body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_input_holds_what_its_generator_says():
    made = mig.build()

    def table(case, kind):
        text = made[mig.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    names = [r[0] for r in csv.reader(io.StringIO(made[mig.INPUT], newline=""))][1:]
    assert len(set(names)) == mig.N_WORKS == 32 and names[-1] == "w00.txt"
    default = table("default", 0)
    assert [r[5] for r in default] == ["20", "8", "8", "14"]
    assert [r[14] for r in default] == ["1", "3", "3", "2"]     # RANK
    assert [r[15] for r in default] == ["4", "3", "", "2"]      # NEXT: 1, 4, 2, 3
    assert default[1][16:19] == ["0", "1000", "0"]              # the same works: tied throughout
    assert default[2][16:19] == ["", "", ""]
    assert all(int(r[6]) <= int(r[7]) <= int(r[8]) for r in default)
    reps = table("default", 1)
    assert len(reps) == 1000 and any(r[1] != r[2] for r in reps)    # inactive works are drawn
    scene = table("scene", 0)
    assert [r[4] for r in scene] == ["4", "7, later", "12", "15"]
    assert scene[3][5:9] == ["0", "0", "0", "0"] and len(table("scene", 1)) == 64
    word = table("word_gap1", 0)
    assert len(word) == 32 and [r for r in word if r[19] == "[?]"][0][1:5] == ["182", "182", "", ""]
    assert len(table("word_gap1", 1)) == 40


def test_word_units_number_the_words_of_the_regions(monkeypatch):
    monkeypatch.setattr(companions.quotes, "find_quotes", oracle_quotes)
    recs = [(w, o, o) for w in (0, 1) for o in range(10, 17) if o != 13]
    cols = [np.array(c, dtype=np.uint32) for c in zip(*recs)]
    labels = {o: ("w%d" % o, "HAN", "4") for _, _, o in recs}
    unit_of, about = companions.word_units_of(labels, *cols, np.zeros(len(recs)), 2, 20, 6, 1, 1, 0)
    assert unit_of.tolist() == [NONE] * 10 + list(range(7)) + [NONE] * 3
    assert about[2] == (12, 12, "HAN", "4", "w12") and about[3] == (13, 13, "", "", "[?]")
    unit_of, about = companions.word_units_of(labels, *cols, np.zeros(len(recs)), 2, 20, 6, 0, 1, 0)
    assert (unit_of == NONE).all() and about == []
    # the restatement's --by word is the same map
    want_of, _ = cr.regions_of(cr.coverage(recs, 2, 6, 1), 20)
    assert [u != NONE for u in want_of] == [o in range(10, 17) for o in range(20)]
