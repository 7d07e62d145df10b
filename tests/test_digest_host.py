"""`ao3.py digest` without a GPU: the oracle's known answers worked by hand
(tests/digest_restated.py), its picks against an independent greedy over bitmasks of Python
ints, the invariants of the contract, the command's refusals, the C ABI's declarations, and the
committed expected CSVs under the product's table-building code with the oracle standing in for
the device."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, digest
from fandom_search_amd.passages import read_matches
from tests import digest_restated as dr
from tests import pairs_restated as plr
from tests.golden import make_digest_golden as mdg
from tests.test_lines_host import works_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE = 0xFFFFFFFF


def pick(work, covered, new_words, new_runs, first, words, cum):
    return dict(work=work, covered=covered, new_words=new_words, new_runs=new_runs,
                longest_first=first, longest_words=words, cum_words=cum)


def work(w, covered, rank, inside, at, best, shared):
    return dict(work=w, covered=covered, pick_rank=rank, in_picks=inside, subsumed_at=at,
                best_pick=best, best_shared=shared)


def invariants(found, works, stopped=False):
    by_work = {v["work"]: v for v in works}
    for r, p in enumerate(found):
        v = by_work[p["work"]]
        assert (v["pick_rank"], v["subsumed_at"], v["best_pick"]) == (r + 1, r + 1, r + 1)
        assert v["best_shared"] == v["covered"] == p["covered"] == v["in_picks"]
        assert p["cum_words"] == sum(q["new_words"] for q in found[:r + 1])
        assert 1 <= p["new_runs"] <= p["new_words"] and p["longest_words"] <= p["new_words"]
    assert [p["new_words"] for p in found] == sorted((p["new_words"] for p in found), reverse=True)
    if not stopped:
        assert all(v["subsumed_at"] != NONE and v["in_picks"] == v["covered"] for v in works)


# ---- oracle known answers, worked by hand ------------------------------------------------

def test_the_second_copy_of_a_work_is_never_picked():
    recs = works_of([[(10, 8)], [(40, 6)], [(10, 8)]])
    found, works, total = dr.digest(recs, 3, 60)
    assert found == [pick(0, 8, 8, 1, 10, 8, 8), pick(1, 6, 6, 1, 40, 6, 14)] and total == 14
    assert works == [work(0, 8, 1, 8, 1, 1, 8), work(1, 6, 2, 6, 2, 2, 6),
                     work(2, 8, NONE, 8, 1, 1, 8)]         # subsumed at the first copy's rank
    invariants(found, works)


def test_a_chain_of_contained_works_gives_one_pick():
    recs = works_of([[(12, 6)], [(10, 10)], [(5, 20)]])    # a inside b inside c
    found, works, total = dr.digest(recs, 3, 60)
    assert found == [pick(2, 20, 20, 1, 5, 20, 20)] and total == 20
    assert [(v["subsumed_at"], v["best_pick"], v["best_shared"]) for v in works] == [
        (1, 1, 6), (1, 1, 10), (1, 1, 20)]


def test_disjoint_works_of_equal_size_come_out_in_first_appearance_order():
    recs = works_of([[(30, 6)], [], [(0, 6)], [(50, 6)], [(10, 6)]])
    found, works, _ = dr.digest(recs, 5, 60)
    assert [p["work"] for p in found] == [0, 2, 3, 4]
    assert [v["work"] for v in works] == [0, 2, 3, 4]      # work 1 has no passage: no row
    invariants(found, works)


def test_new_words_in_two_runs_the_longest_first_among_equals():
    # work 0 takes 20..29; work 1 covers 15..34: five new words on either side
    recs = works_of([[(20, 10)], [(15, 20)]])
    found, works, _ = dr.digest(recs, 2, 60)
    assert found == [pick(1, 20, 20, 1, 15, 20, 20)]       # the larger work comes first
    recs = works_of([[(20, 12)], [(15, 10), (27, 10)]])    # 15..24 and 27..36 against 20..31
    found, works, _ = dr.digest(recs, 2, 60)
    assert found == [pick(1, 20, 20, 2, 15, 10, 20), pick(0, 12, 2, 1, 25, 2, 22)]
    recs = works_of([[(20, 13)], [(15, 10), (28, 10)]])    # new for work 1: 15..19 and 33..37
    found, works, _ = dr.digest(recs, 2, 60)
    assert found[1] == pick(0, 13, 3, 1, 25, 3, 23)
    recs = works_of([[(20, 14)], [(15, 10)], [(29, 10)], [(15, 10), (29, 10)]])
    found, works, _ = dr.digest(recs, 4, 60)               # work 3: 20 words; then work 0: 4
    assert found == [pick(3, 20, 20, 2, 15, 10, 20), pick(0, 14, 4, 1, 25, 4, 24)]
    assert works[1] == work(1, 10, NONE, 10, 1, 1, 10) and works[0]["best_shared"] == 14


def test_a_bridged_word_counts_under_max_gap_one():
    recs = [(0, k, 10 + k) for k in range(3)] + [(0, 4 + k, 14 + k) for k in range(3)]
    found, works, total = dr.digest(recs, 1, 30, min_words=6, max_gap=1)
    assert found == [pick(0, 7, 7, 1, 10, 7, 7)] and total == 7
    assert dr.digest(recs, 1, 30, min_words=6, max_gap=0) == ([], [], 0)


def test_each_stop_rule_fires_exactly_at_its_bound_and_not_one_short_of_it():
    recs = works_of([[(20 * k, 10 - k)] for k in range(5)])    # gains 10, 9, 8, 7, 6: TOTAL 40
    n = lambda **kw: len(dr.digest(recs, 5, 200, **kw)[0])     # noqa: E731
    assert n() == 5
    assert [n(picks=k) for k in (1, 4, 5, 6)] == [1, 4, 5, 5]
    assert [n(min_gain=g) for g in (6, 7, 10, 11)] == [5, 4, 1, 0]
    # |K| * 100 >= P * 40 after 10, 19, 27, 34 words: 25 % stops at 10, 26 % needs 19
    assert [n(cover=p) for p in (1, 25, 26, 47, 48, 85, 86, 100)] == [1, 1, 2, 2, 3, 4, 5, 5]
    found, works, _ = dr.digest(recs, 5, 200, cover=48)
    assert [v["subsumed_at"] for v in works] == [1, 2, 3, NONE, NONE]
    assert [v["best_pick"] for v in works] == [1, 2, 3, NONE, NONE]
    invariants(found, works, stopped=True)
    for bad in (dict(min_words=0), dict(min_gain=0), dict(cover=0), dict(cover=101),
                dict(picks=-1)):
        with pytest.raises(ValueError):
            dr.digest(recs, 5, 200, **bad)
    with pytest.raises(ValueError):
        dr.digest(recs, 4, 200)
    with pytest.raises(ValueError):
        dr.digest(recs, 5, 80)


# ---- the greedy loop against another one -------------------------------------------------

def greedy_over_ints(cov, picks, cover, min_gain):
    """[(work, gain)] by a greedy over one Python int per work, a bit per script word."""
    masks = [sum(1 << o for o in words) for words in cov]
    every = 0
    for m in masks:
        every |= m
    total, have, out = bin(every).count("1"), 0, []
    while True:
        if picks and len(out) == picks:
            break
        best_w, best_g = None, 0
        for w, m in enumerate(masks):                      # strictly more: the earlier on a tie
            g = bin(m & ~have).count("1")
            if g > best_g:
                best_w, best_g = w, g
        if best_g < min_gain or bin(have).count("1") * 100 >= cover * total:
            break
        out.append((best_w, best_g))
        have |= masks[best_w]
    return out


def random_records(rng, n_works, n_script):
    spans_of = [[(int(rng.integers(0, n_script - 8)), int(rng.integers(2, 9)))
                 for _ in range(int(rng.integers(0, 4)))] for _ in range(n_works)]
    return works_of(spans_of)


def test_the_picks_are_those_of_a_greedy_over_bitmasks():
    rng = np.random.default_rng(7)
    made = stopped = 0
    for case in range(300):
        n_works, n_script = int(rng.integers(1, 14)), int(rng.integers(10, 61))
        recs = random_records(rng, n_works, n_script)
        picks = int(rng.integers(0, 4)) if case % 3 == 0 else 0
        cover = int(rng.integers(1, 101)) if case % 3 == 1 else 100
        gain = int(rng.integers(1, 6)) if case % 3 == 2 else 1
        found, works, total = dr.digest(recs, n_works, n_script, 2, 0, picks, cover, gain)
        cov = plr.coverage(recs, n_works, 2, 0)
        assert [(p["work"], p["new_words"]) for p in found] == greedy_over_ints(
            cov, picks, cover, gain), case
        full = bool(found) and found[-1]["cum_words"] == total
        invariants(found, works, stopped=not full)
        assert len(found) <= min(len(works), total)
        # a word's stamp is the first pick holding it: subsumed_at by the picks' coverage
        for v in works:
            k = next((k for k in range(1, len(found) + 1)
                      if cov[v["work"]] <= set().union(*[cov[p["work"]] for p in found[:k]])),
                     NONE)
            assert v["subsumed_at"] == k, case
        made += len(found)
        stopped += not full
    assert made > 300 and stopped > 60                     # (the cases are not empty ones)


# ---- the command's surface ----------------------------------------------------------------

@pytest.mark.parametrize("bad,message", [
    (["--min-words", "0"], "--min-words and --min-gain must be at least 1, --max-gap and --picks "
                           "at least 0"),
    (["--min-gain", "0"], "--min-words and --min-gain must be at least 1, --max-gap and --picks "
                          "at least 0"),
    (["--max-gap", "-1"], "--min-words and --min-gain must be at least 1, --max-gap and --picks "
                          "at least 0"),
    (["--picks", "-1"], "--min-words and --min-gain must be at least 1, --max-gap and --picks "
                        "at least 0"),
    (["--cover", "0"], "--cover must be from 1 to 100"),
    (["--cover", "101"], "--cover must be from 1 to 100")])
def test_bad_arguments_exit_with_an_error_line(bad, message, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["digest", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code) == "ao3.py digest: error: " + message


def test_parser_defaults_and_output_names():
    args = cli.ao3_parser().parse_args(["digest", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_digest"
    assert (args.output, args.min_words, args.max_gap, args.picks, args.cover, args.min_gain,
            args.device, args.reader) == (None, 6, 0, 0, 100, 1, 0, None)
    assert digest.output_names(args.matches) == (
        "runs/match-6gram-20240101-digest.csv", "runs/match-6gram-20240101-digest-works.csv")
    assert digest.output_names("m.csv", "out/x")[1] == "out/x-digest-works.csv"
    args = cli.ao3_parser().parse_args(
        ["digest", "m.csv", "-o", "p", "--min-words", "3", "--max-gap", "2", "--picks", "4",
         "--cover", "80", "--min-gain", "5", "--device", "1", "--reader", "python"])
    assert (args.output, args.min_words, args.max_gap, args.picks, args.cover, args.min_gain,
            args.device, args.reader) == ("p", 3, 2, 4, 80, 5, 1, "python")
    assert (digest.PICK_FIELDS, digest.WORK_FIELDS) == (dr.PICK_FIELDS, dr.WORK_FIELDS)
    assert "digest" in cli.ao3_parser().format_help()
    # the parsers whose surfaces are pinned do not know the command
    with pytest.raises(SystemExit):
        cli.full_parser().parse_args(["digest", "m.csv"])


# ---- the C ABI ---------------------------------------------------------------------------

def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_digest", "fs_digest_rows", "fs_digest_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)
    assert "digest" in _lib.TIMED
    assert abi.DIGEST_MS_NAMES == ("coverage", "rounds", "works", "total", "rounds_enqueued",
                                   "tiles_read")
    assert re.search(r"#define FS_DIGEST_MAX_BYTES \(1u << 30\)", text)
    assert abi.FS_DIGEST_MAX_BYTES == 1 << 30


@pytest.mark.parametrize("struct,dtype,keys", [
    ("fs_digest_pick", "DIGEST_PICK_DTYPE", dr.PICK_KEYS + ["reserved"]),
    ("fs_digest_work", "DIGEST_WORK_DTYPE", dr.WORK_KEYS + ["reserved"])])
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
    n_picks, n_active, total = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    u32 = abi.ptr(z, C.c_uint32)
    found = np.ones(2, dtype=abi.DIGEST_PICK_DTYPE)
    works = np.ones(2, dtype=abi.DIGEST_WORK_DTYPE)
    pp, wp = (x.ctypes.data_as(C.c_void_p) for x in (found, works))

    def call(n_rows=1, n_script=4, min_words=1, picks=0, cover=100, min_gain=1, p_out=pp,
             p_cap=2, np_=C.byref(n_picks), w_out=wp, w_cap=2, na=C.byref(n_active),
             tot=C.byref(total), cols=u32):
        return L.fs_digest(0, cols, cols, cols, n_rows, 1, n_script, min_words, 0, picks, cover,
                           min_gain, p_out, p_cap, np_, w_out, w_cap, na, tot)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_gain=0) == abi.FS_E_INVALID
    assert call(cover=0) == abi.FS_E_INVALID
    assert call(cover=101) == abi.FS_E_INVALID
    assert b"1 to 100" in L.fs_last_error()
    assert call(cover=0, n_rows=1 << 32) == abi.FS_E_INVALID   # invalid before unsupported
    assert call(p_out=None) == abi.FS_E_INVALID                # a capacity without a buffer
    assert call(w_out=None) == abi.FS_E_INVALID
    assert call(np_=None) == abi.FS_E_INVALID
    assert call(na=None) == abi.FS_E_INVALID
    assert call(tot=None) == abi.FS_E_INVALID
    assert call(cols=None) == abi.FS_E_INVALID
    assert (n_picks.value, n_active.value, total.value) == (0, 0, 0)   # (cleared behind the flags)
    n_picks.value = n_active.value = total.value = 7
    # no records: no picks and no works, no device work
    assert call(n_rows=0, cols=None, p_out=None, p_cap=0, w_out=None, w_cap=0) == abi.FS_OK
    assert (n_picks.value, n_active.value, total.value) == (0, 0, 0)
    assert (found["covered"] == 1).all() and (works["covered"] == 1).all()   # nothing written
    assert L.fs_digest_times(None) == abi.FS_E_INVALID
    assert L.fs_digest_rows(None, None, 0, 0, 1, 0, 0, 100, 1, None, 0, C.byref(n_picks), None, 0,
                            C.byref(n_active), C.byref(total)) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        digest.find_digest(z, z[:3], z, 1, 4)              # columns of different lengths


def test_flags_the_tables_refuse_before_the_library_is_asked(monkeypatch):
    def never(*a, **k):
        raise AssertionError("the library was asked")
    monkeypatch.setattr(digest, "find_digest", never)
    rows = read_matches(os.path.join(GOLDEN, mdg.INPUT))
    for kw in (dict(min_words=0), dict(min_gain=0), dict(cover=0), dict(cover=101),
               dict(picks=-1)):
        with pytest.raises(ValueError):
            digest.tables(rows, **kw)


# ---- committed expected outputs ---------------------------------------------------------

def oracle_find(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0, picks=0,
                cover=100, min_gain=1, device=0):
    recs = list(zip(*(np.asarray(c).tolist() for c in (work, fan_ix, orig_ix))))
    found, works, total = dr.digest(recs, n_works, n_script, min_words, max_gap, picks, cover,
                                    min_gain)
    return (np.array([tuple(r[k] for k in dr.PICK_KEYS) + (0,) for r in found],
                     dtype=abi.DIGEST_PICK_DTYPE),
            np.array([tuple(r[k] for k in dr.WORK_KEYS) + (0,) for r in works],
                     dtype=abi.DIGEST_WORK_DTYPE), total)


def test_the_golden_generator_reproduces_its_committed_files():
    made = mdg.build()
    assert set(made) == {mdg.INPUT} | {n for c in mdg.CASES for n in mdg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


@pytest.mark.parametrize("case,min_words,max_gap,picks,cover,min_gain", mdg.CASES)
def test_the_tables_under_the_oracle_give_the_goldens(monkeypatch, case, min_words, max_gap,
                                                      picks, cover, min_gain):
    monkeypatch.setattr(digest, "find_digest", oracle_find)
    body = digest.tables(read_matches(os.path.join(GOLDEN, mdg.INPUT)), min_words, max_gap,
                         picks, cover, min_gain)
    heads = (digest.PICK_FIELDS, digest.WORK_FIELDS)
    for name, head, part in zip(mdg.golden_names(case), heads, body):
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([head] + part)
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert buf.getvalue().encode("utf-8") == fh.read(), name


def test_the_golden_files_hold_what_their_generator_says():
    made = mdg.build()

    def table(case, kind):
        text = made[mdg.golden_names(case)[kind]]
        return [r for r in csv.reader(io.StringIO(text, newline=""))][1:]
    picks, works = table("default", 0), table("default", 1)
    # a before its copy b; d's two passages are two new runs; e and k add three words each and e
    # comes first in the file; l's one word ends it at 100 %
    assert [(r[1], r[3], r[4]) for r in picks] == [("a.txt", "16", "1"), ("d.txt", "13", "2"),
                                                   ("h.txt", "10", "1"), ("e.txt", "3", "1"),
                                                   ("dir/l.txt", "1", "1")]
    assert [r[11] for r in picks] == ["37", "67", "90", "97", "100"] and picks[-1][10] == "43"
    assert sum(int(r[12]) for r in picks) == len(works) == 11 == int(picks[-1][13])
    assert sum(int(r[14]) for r in picks) == 11
    by_name = {r[0]: r for r in works}
    assert by_name["b.txt"][2:] == ["", "16", "100", "1", "1", "a.txt", "16"]
    assert by_name["c.txt"][5:8] == ["1", "1", "a.txt"]                # contained in a
    assert by_name["k.txt"][5:] == ["4", "3", "h.txt", "7"]            # e's words complete it
    assert "i.txt" not in by_name                                      # no passage
    # --max-gap 1: h's run holds the word no record names; 80 % is passed at the third pick
    gap1 = table("gap1_cover80", 0)
    assert [(r[1], r[11]) for r in gap1] == [("a.txt", "33"), ("h.txt", "64"), ("d.txt", "91")]
    assert gap1[1][15] == ("the quality of mercy [?] not strained it droppeth as the gentle rain "
                           "from heaven")
    unfinished = [r[0] for r in table("gap1_cover80", 1) if r[5] == ""]
    assert unfinished == ["e.txt", "k.txt", "dir/l.txt"]
    assert [r[:14] for r in table("picks2", 0)] == [r[:14] for r in picks[:2]]
    assert [r[14] for r in table("picks2", 0)] == ["4", "4"]   # k is most like a now, e like d
    assert [r for r in table("picks2", 1) if r[0] == "h.txt"] == [
        ["h.txt", "10", "", "0", "0", "", "", "", "0"]]


def test_no_records_give_two_header_only_files(tmp_path, monkeypatch):
    monkeypatch.setattr(digest, "find_digest", oracle_find)
    src = tmp_path / "m.csv"
    with open(os.path.join(GOLDEN, mdg.INPUT), newline="", encoding="utf-8") as fh:
        src.write_text(fh.readline(), encoding="utf-8")
    assert cli.main(["digest", str(src), "--reader", "python"]) == 0
    outs = digest.output_names(str(src))
    assert open(outs[0]).read().split() == [",".join(digest.PICK_FIELDS)]
    assert open(outs[1]).read().split() == [",".join(digest.WORK_FIELDS)]
    assert dr.digest_csv(src.read_text(encoding="utf-8")) == tuple(
        open(p, newline="", encoding="utf-8").read() for p in outs)
