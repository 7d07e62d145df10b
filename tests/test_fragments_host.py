"""`ao3.py fragments` without a GPU: the oracle's known answers worked by hand
(tests/fragments_restated.py), the START/END table identity the library rests on against the
oracle's work-by-work counts, the cross-properties of the two outputs, the command's refusals,
the C ABI's declarations, and the committed expected CSVs under the product's table-building
code with the oracle standing in for the device."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, fragments
from fandom_search_amd.passages import read_matches
from tests import fragments_restated as fr
from tests import pairs_restated as plr
from tests.golden import make_fragments_golden as mfg
from tests.test_lines_host import works_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def frag(first, last, works, exact, start, end, first_work):
    return dict(first=first, last=last, works=works, exact_works=exact, start_works=start,
                end_works=end, first_work=first_work)


def work(w, runs, covered, held, exact, lf, ll, lw):
    return dict(work=w, runs=runs, covered=covered, held=held, exact=exact, longest_first=lf,
                longest_last=ll, longest_works=lw)


# ---- oracle known answers, worked by hand ------------------------------------------------

def test_a_phrase_nested_in_a_longer_one_with_different_supports():
    # works 0, 1: the whole message 10..21; works 2, 3, 4: only its words 13..17
    recs = works_of([[(10, 12)], [(10, 12)], [(13, 5)], [(13, 5)], [(13, 5)]])
    found, works = fr.fragments(recs, 5, 30, min_words=3)
    assert found == [frag(13, 17, 5, 3, 3, 3, 2), frag(10, 21, 2, 2, 2, 2, 0)]
    assert works == [work(0, 1, 12, 2, 1, 10, 21, 2), work(1, 1, 12, 2, 1, 10, 21, 2),
                     work(2, 1, 5, 1, 1, 13, 17, 5), work(3, 1, 5, 1, 1, 13, 17, 5),
                     work(4, 1, 5, 1, 1, 13, 17, 5)]
    # only the inner phrase reaches three works
    found, works = fr.fragments(recs, 5, 30, min_words=3, min_works=3)
    assert found == [frag(13, 17, 5, 3, 3, 3, 2)]
    assert [w["held"] for w in works] == [1] * 5 and [w["exact"] for w in works] == [0, 0, 1, 1, 1]


def test_two_abutting_passages_of_one_work_make_one_run():
    # work 0 quotes 10..15 and 16..21 in two passages; work 1 quotes 10..21 in one
    recs = works_of([[(10, 6), (16, 6)], [(10, 12)]])
    found, works = fr.fragments(recs, 2, 30, min_words=3)
    assert found == [frag(10, 21, 2, 2, 2, 2, 0)]            # no passage of work 0 holds it
    assert works[0] == work(0, 1, 12, 1, 1, 10, 21, 2)
    # a word between the two passages: two runs, and no stretch two works hold
    recs = works_of([[(10, 6), (17, 5)], [(10, 12)]])
    found, works = fr.fragments(recs, 2, 30, min_words=3)
    assert [(f["first"], f["last"]) for f in found] == [(17, 21), (10, 15)]
    assert works[0] == work(0, 2, 11, 2, 2, 10, 15, 2)


def test_a_fragment_at_word_zero_and_one_at_the_script_s_last_word():
    recs = works_of([[(0, 4), (26, 4)], [(0, 5), (25, 5)]])
    found, _ = fr.fragments(recs, 2, 30, min_words=3)
    assert found == [frag(0, 3, 2, 1, 2, 1, 0), frag(26, 29, 2, 1, 1, 2, 0)]


def test_a_bridged_word_counts_under_max_gap_one():
    # work 0 has no record of word 13
    recs = [(0, k, 10 + k) for k in range(3)] + [(0, 4 + k, 14 + k) for k in range(3)]
    recs += [(1, k, 10 + k) for k in range(7)]
    found, works = fr.fragments(recs, 2, 30, min_words=6, max_gap=1)
    assert found == [frag(10, 16, 2, 2, 2, 2, 0)] and works[0]["covered"] == 7
    found, works = fr.fragments(recs, 2, 30, min_words=6, max_gap=0)
    assert found == [] and [w["work"] for w in works] == [1]


def test_a_work_that_repeats_a_line_counts_once():
    recs = works_of([[(10, 6), (10, 6), (10, 6)], [(10, 6)]])
    found, works = fr.fragments(recs, 2, 30, min_words=3)
    assert found == [frag(10, 15, 2, 2, 2, 2, 0)]
    assert works[0] == work(0, 1, 6, 1, 1, 10, 15, 2)


def test_max_words_is_no_closure():
    # works 0, 1 quote ten words: under max_words 8 no stretch of eight is closed and the ten
    # are not listed; the longest run is outside the lengths
    recs = works_of([[(10, 10)], [(10, 10)], [(12, 3)]])
    found, works = fr.fragments(recs, 3, 30, min_words=3, max_words=8)
    assert found == [frag(12, 14, 3, 1, 1, 1, 2)]
    assert [w["longest_works"] for w in works] == [NONE, NONE, 3]
    assert [w["held"] for w in works] == [1, 1, 1]


# ---- the table method against the definition ----------------------------------------------

def by_tables(cov, n_script, min_works, min_length, max_words):
    """{(first, last): (S, START, END)} of the listed cells by the START/END tables."""
    out = {}
    runs = [r for words in cov for r in fr.runs_of(words)]
    for d in range(min_length - 1, max_words):
        start, end = [0] * (n_script + 1), [0] * (n_script + 1)
        for f, l in runs:
            if d <= l - f:
                start[f] += 1
                end[l - d] += 1
        s = 0
        for a in range(n_script):
            s += start[a]
            if start[a] and end[a] and s >= min_works:
                out[(a, a + d)] = (s, start[a], end[a])
            s -= end[a]
    return out


def random_records(rng, n_works, n_script):
    spans_of = [[(int(rng.integers(0, n_script - 8)), int(rng.integers(2, 9)))
                 for _ in range(int(rng.integers(0, 4)))] for _ in range(n_works)]
    return works_of(spans_of)


def test_the_start_end_identity_gives_the_closed_intervals_of_the_definition():
    rng = np.random.default_rng(5)
    some = 0
    for case in range(300):
        n_works, n_script = int(rng.integers(1, 9)), int(rng.integers(10, 41))
        recs = random_records(rng, n_works, n_script)
        k, lo = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        hi = lo + int(rng.integers(0, 12))
        found, works = fr.fragments(recs, n_works, n_script, 2, 0, k, lo, hi)
        cov = plr.coverage(recs, n_works, 2, 0)
        table = by_tables(cov, n_script, k, lo, hi)
        assert {(f["first"], f["last"]): (f["works"], f["start_works"], f["end_works"])
                for f in found} == table, case
        # what the works hold is what the fragments are held by
        assert sum(w["held"] for w in works) == sum(f["works"] for f in found)
        assert sum(w["exact"] for w in works) == sum(f["exact_works"] for f in found)
        some += len(found)
    assert some > 300                                      # (the cases are not empty ones)


def test_every_run_is_a_fragment_under_the_loosest_flags():
    rng = np.random.default_rng(6)
    for case in range(50):
        n_works, n_script = int(rng.integers(1, 9)), int(rng.integers(10, 41))
        recs = random_records(rng, n_works, n_script)
        found, works = fr.fragments(recs, n_works, n_script, 2, 0, 1, 1, n_script)
        listed = {(f["first"], f["last"]) for f in found}
        cov = plr.coverage(recs, n_works, 2, 0)
        runs = {r for words in cov for r in fr.runs_of(words)}
        assert runs <= listed
        assert all(w["exact"] == w["runs"] for w in works)
        # and a fragment that is no run is where runs of different works overlap
        for a, b in listed - runs:
            assert any(f <= a and b <= l and (f, l) != (a, b) for f, l in runs)


# ---- the command's surface ----------------------------------------------------------------

@pytest.mark.parametrize("bad,message", [
    (["--min-words", "0"], "--min-words, --min-works and --min-length must be at least 1, "
                           "--max-gap and --top at least 0"),
    (["--min-works", "0"], "--min-words, --min-works and --min-length must be at least 1, "
                           "--max-gap and --top at least 0"),
    (["--min-length", "0"], "--min-words, --min-works and --min-length must be at least 1, "
                            "--max-gap and --top at least 0"),
    (["--max-gap", "-1"], "--min-words, --min-works and --min-length must be at least 1, "
                          "--max-gap and --top at least 0"),
    (["--top", "-1"], "--min-words, --min-works and --min-length must be at least 1, "
                      "--max-gap and --top at least 0"),
    (["--max-words", "2"], "--max-words must be from --min-length to 4096"),
    (["--max-words", "4097"], "--max-words must be from --min-length to 4096")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["fragments", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py fragments: error: " + message


def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["fragments", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_fragments"
    assert (args.output, args.min_words, args.max_gap, args.min_works, args.min_length,
            args.max_words, args.top, args.device, args.reader) == (None, 6, 0, 2, 3, 128, 0, 0,
                                                                    None)
    assert fragments.output_names(args.matches) == (
        "runs/match-6gram-20240101-fragments.csv",
        "runs/match-6gram-20240101-fragments-works.csv")
    assert fragments.output_names("m.csv", "out/x")[1] == "out/x-fragments-works.csv"
    args = cli.ao3_parser().parse_args(
        ["fragments", "m.csv", "-o", "p", "--min-words", "3", "--max-gap", "2", "--min-works",
         "4", "--min-length", "2", "--max-words", "9", "--top", "5", "--device", "1", "--reader",
         "python"])
    assert (args.output, args.min_words, args.max_gap, args.min_works, args.min_length,
            args.max_words, args.top, args.device, args.reader) == ("p", 3, 2, 4, 2, 9, 5, 1,
                                                                    "python")
    assert (fragments.FRAGMENT_FIELDS, fragments.WORK_FIELDS) == (fr.FRAGMENT_FIELDS,
                                                                  fr.WORK_FIELDS)
    assert "fragments" in cli.ao3_parser().format_help()
    # the parsers whose surfaces are pinned do not know the command
    with pytest.raises(SystemExit):
        cli.full_parser().parse_args(["fragments", "m.csv"])


def test_the_ranking_is_works_then_words_then_the_first_word():
    frags = np.zeros(5, dtype=abi.FRAGMENT_DTYPE)          # in (words, first) order
    frags["first"] = [7, 20, 3, 9, 1]
    frags["last"] = [9, 22, 7, 13, 10]
    frags["works"] = [4, 4, 9, 4, 2]
    assert fragments.rank_order(frags).tolist() == [2, 3, 0, 1, 4]


# ---- the C ABI ---------------------------------------------------------------------------

def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_fragments", "fs_fragments_rows", "fs_fragments_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert abi.FRAGMENTS_MS_NAMES == ("runs", "spread", "list", "works", "total")
    assert re.search(r"#define FS_FRAGMENTS_MAX_BYTES \(1u << 30\)", text)
    assert re.search(r"#define FS_FRAGMENTS_MAX_WORDS 4096u", text)
    assert abi.FS_FRAGMENTS_MAX_BYTES == 1 << 30 and abi.FS_FRAGMENTS_MAX_WORDS == 4096


@pytest.mark.parametrize("struct,dtype,keys", [
    ("fs_fragment", "FRAGMENT_DTYPE", fr.FRAGMENT_KEYS + ["reserved"]),
    ("fs_fragment_work", "FRAGMENT_WORK_DTYPE", fr.WORK_KEYS)])
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
    assert dt.itemsize == at == 32
    assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n_frags, n_active = C.c_uint64(7), C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    frags = np.ones(2, dtype=abi.FRAGMENT_DTYPE)
    works = np.ones(2, dtype=abi.FRAGMENT_WORK_DTYPE)
    fp, wp = (x.ctypes.data_as(C.c_void_p) for x in (frags, works))

    def call(n_rows=1, n_script=4, min_words=1, min_length=3, max_words=128, f_out=fp, f_cap=2,
             nf=C.byref(n_frags), w_out=wp, w_cap=2, na=C.byref(n_active), cols=u32):
        return L.fs_fragments(0, cols, cols, cols, n_rows, 1, n_script, min_words, 0, 2,
                              min_length, max_words, f_out, f_cap, nf, w_out, w_cap, na)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(max_words=4097) == abi.FS_E_UNSUPPORTED
    assert b"4096" in L.fs_last_error()
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_length=0) == abi.FS_E_INVALID
    assert call(min_length=4, max_words=3) == abi.FS_E_INVALID
    assert call(min_length=5000, max_words=4097) == abi.FS_E_INVALID   # invalid before unsupported
    assert call(f_out=None) == abi.FS_E_INVALID                # a capacity without a buffer
    assert call(w_out=None) == abi.FS_E_INVALID
    assert call(nf=None) == abi.FS_E_INVALID
    assert call(na=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (n_frags.value, n_active.value) == (0, 0)           # (cleared once the flags passed)
    n_frags.value = n_active.value = 7
    # no records: no fragments and no works, no device work
    assert call(n_rows=0, cols=None, f_out=None, f_cap=0, w_out=None, w_cap=0) == abi.FS_OK
    assert (n_frags.value, n_active.value) == (0, 0)
    assert (frags["works"] == 1).all() and (works["runs"] == 1).all()  # nothing written
    assert L.fs_fragments_times(None) == abi.FS_E_INVALID
    assert L.fs_fragments_rows(None, None, 0, 0, 1, 0, 2, 3, 128, None, 0, C.byref(n_frags),
                               None, 0, C.byref(n_active)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        fragments.find_fragments(z, z[:3], z, 1, 4)            # columns of different lengths


def test_flags_the_tables_refuse_before_the_library_is_asked(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was asked")
    monkeypatch.setattr(fragments, "find_fragments", never)
    rows = read_matches(os.path.join(GOLDEN, mfg.INPUT))
    for kw in (dict(min_words=0), dict(min_works=0), dict(min_length=0),
               dict(min_length=4, max_words=3), dict(max_words=4097)):
        with pytest.raises(ValueError):
            fragments.tables(rows, **kw)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0, min_works=2,
                min_length=3, max_words=128, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    found, works = fr.fragments(recs, n_works, n_script, min_words, max_gap, min_works,
                                min_length, max_words)
    return (np.array([tuple(r[k] for k in fr.FRAGMENT_KEYS) + (0,) for r in found],
                     dtype=abi.FRAGMENT_DTYPE),
            np.array([tuple(r[k] for k in fr.WORK_KEYS) for r in works],
                     dtype=abi.FRAGMENT_WORK_DTYPE))


def test_the_golden_generator_reproduces_its_committed_files():
    made = mfg.build()
    assert set(made) == {mfg.INPUT} | {n for c in mfg.CASES for n in mfg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,min_words,max_gap,min_works,min_length,max_words,top", mfg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, min_words, max_gap,
                                                      min_works, min_length, max_words, top):
    monkeypatch.setattr(fragments, "find_fragments", oracle_find)
    body = fragments.tables(read_matches(os.path.join(GOLDEN, mfg.INPUT)), min_words, max_gap,
                            min_works, min_length, max_words, top)
    heads = (fragments.FRAGMENT_FIELDS, fragments.WORK_FIELDS)
    for name, head, part in zip(mfg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_files_hold_what_their_generator_says():
    made = mfg.build()

    def table(case, kind):
        text = made[mfg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    default = table("default", 0)
    # the five words in the middle of "i have a bad feeling about this": four works, nested in
    # stretches of three works and of two
    assert [(r[1], r[2], r[6]) for r in default][:4] == [("62", "67", "4"), ("5", "9", "4"),
                                                         ("4", "9", "3"), ("5", "10", "3")]
    assert [r[0] for r in default] == [str(k + 1) for k in range(len(default))]
    assert default[0][11] == "may the force be with you" and default[0][7] == "4"  # c: once
    assert [(r[1], r[2]) for r in default if r[1] == "0"] == [("0", "9")]          # word 0
    # e.txt quotes the long line in two passages that abut: one run, a fragment of two works
    carpet = [r for r in default if r[3] == "14"]
    assert [(r[6], r[7], r[10]) for r in carpet] == [("2", "2", "e.txt")]
    assert [r[1] for r in table("default", 1) if r[0] == "e.txt"] == ["1"]
    assert not [r for r in table("default", 1) if r[0] in ("f.txt", "h.txt", "j.txt")]
    gap1 = table("gap1_min1", 0)
    smell = [r for r in gap1 if r[10] == "f.txt"]
    assert [(r[6], r[11]) for r in smell] == [("2", "what an incredible [?] you have discovered")]
    assert table("top3", 0) == default[:3] and table("top3", 1) == table("default", 1)


def test_no_records_give_two_header_only_files(tmp_path, monkeypatch):
    monkeypatch.setattr(fragments, "find_fragments", oracle_find)
    src = tmp_path / "m.csv"
    with open(os.path.join(GOLDEN, mfg.INPUT), newline="", encoding="utf-8") as fh:
        src.write_text(fh.readline(), encoding="utf-8")
    assert cli.main(["fragments", str(src), "--reader", "python"]) == 0
    outs = fragments.output_names(str(src))
    assert open(outs[0]).read().split() == [",".join(fragments.FRAGMENT_FIELDS)]
    assert open(outs[1]).read().split() == [",".join(fragments.WORK_FIELDS)]
    assert fr.fragments_csv(src.read_text(encoding="utf-8")) == tuple(
        open(p, newline="", encoding="utf-8").read() for p in outs)
