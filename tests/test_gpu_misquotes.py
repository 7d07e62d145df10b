"""`ao3.py misquotes` on the GPU: fs_misquotes against its plain-Python restatement
(tests/misquotes_restated.py), every field of the three record arrays, with every table's hash
whole, cut to 4 bits and cut to nothing; one long posting list against its closed form; the
caps, the bound and the refusals; a cross-check against fs_variants; and the command under both
readers against the committed expected CSVs."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, misquotes, variants
from fandom_search_amd.cli import main
from tests import misquotes_restated as mr
from tests.golden import make_misquotes_golden as mmg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = 0xFFFFFFFF
FAN_GAP = 10                # fan words between two quotations of a work: they never join
LINE = 8                    # words of a line of the synthetic script, lines 10 words apart
WRONG = 100_000             # spellings from here on are nobody's script word


@pytest.fixture(autouse=True)
def no_diagnostics(monkeypatch):
    monkeypatch.delenv("FS_MISQUOTES_HASH_BITS", raising=False)
    monkeypatch.delenv("FS_MISQUOTES_MAX_PAIRS", raising=False)


def layout(quotes):
    """Columns (work, fan_ix, orig_ix, spell), sorted by (work, fan_ix), of the quotations
    (work, orig_first, spells; None: no record for that script word) laid out one behind another
    in their work."""
    cols = [[], [], [], []]
    at = {}
    for work, orig, spells in sorted(quotes, key=lambda q: q[0]):           # stable
        fan = at.get(work, 0)
        for j, s in enumerate(spells):
            if s is not None:
                for c, v in zip(cols, (work, fan + j, orig + j, s)):
                    c.append(v)
        at[work] = fan + len(spells) + FAN_GAP
    return [np.asarray(c, dtype=np.uint32) for c in cols]


def verbatim(o0, n=LINE, **changed):
    """The spellings of n script words from o0 on, each spelt as itself (script word o is
    spelling o), those at the offsets `changed` names (w0, w1, ...) replaced."""
    spells = [o0 + k for k in range(n)]
    for k, s in changed.items():
        spells[int(k[1:])] = s
    return spells


def script_same(n_script):
    """same[]: script word o is spelling o, and every 37th word has no spelling of its own."""
    same = np.arange(n_script, dtype=np.uint32)
    same[5::37] = NONE
    return same


def check(cols, same, n_works, n_spell, **kw):
    """fs_misquotes against the restatement; returns (works, misquotes, pairs)."""
    works, found, pairs = misquotes.find_misquotes(*cols, same, n_works, n_spell, **kw)
    want_w, want_m, want_p = mr.misquotes(list(zip(*(c.tolist() for c in cols))), same.tolist(),
                                          n_works, n_spell, **kw)
    assert (len(works), len(found), len(pairs)) == (len(want_w), len(want_m), len(want_p))
    assert (works.dtype, found.dtype, pairs.dtype) == (
        abi.MISQUOTE_WORK_DTYPE, abi.MISQUOTE_DTYPE, abi.MISQUOTE_PAIR_DTYPE)
    for got, want, keys in ((found, want_m, mr.MISQUOTE_KEYS), (works, want_w, mr.WORK_KEYS),
                            (pairs, want_p, mr.PAIR_KEYS)):
        assert list(got.dtype.names) == keys
        for name in keys:
            assert got[name].tolist() == [d[name] for d in want], name
    return works, found, pairs


def fandom(rng, n_active, n_lines=12):
    """(cols, same, n_works, n_spell): `n_active` works that each quote some of the lines, in
    families of 2 to 5 that copy one to three misquotes of a line all of them quote; a misquote
    most works have; one-off typos; a work that steps over a word; a run one word short; and
    three works without any passage."""
    n_script = 10 * n_lines + 10
    quotes, wrong = [], WRONG
    lines_of = [sorted(rng.choice(n_lines, size=int(rng.integers(2, 5)), replace=False).tolist())
                for _ in range(n_active)]
    changed = [dict() for _ in range(n_active)]               # (line, offset): spelling
    w = 0
    while w < n_active:
        size = min(int(rng.integers(2, 6)), n_active - w)
        line = int(rng.integers(0, n_lines))
        for _ in range(int(rng.integers(1, 4))):
            k, wrong = int(rng.integers(0, LINE)), wrong + 1
            for member in range(w, w + size):
                if line not in lines_of[member]:
                    lines_of[member] = sorted(lines_of[member] + [line])
                changed[member][(line, k)] = wrong
        w += size
    for w in range(n_active):
        for line in lines_of[w]:
            spells = verbatim(10 * line)
            if line == 0 and w % 4:                           # most readers of word 3
                spells[3] = WRONG
            for k in range(LINE):
                if (line, k) in changed[w]:
                    spells[k] = changed[w][(line, k)]
                elif rng.random() < 0.02:
                    wrong += 1
                    spells[k] = wrong                         # a one-off
            if w % 7 == 3 and line == lines_of[w][0]:
                spells[4] = None                              # two runs, one under --max-gap 1
            quotes.append((w, 10 * line, spells))
        if w % 5 == 1:
            quotes.append((w, 10 * n_lines, verbatim(10 * n_lines, 5, w1=WRONG + 1)))
    n_works = n_active + 3
    quotes.append((n_active, 10, verbatim(10, 5, w2=WRONG + 1)))         # too short: not active
    quotes.append((n_active + 2, 20, verbatim(20, 3)))
    return layout(quotes), script_same(n_script), n_works, wrong + 1


OPTIONS = [dict(), dict(min_works=3), dict(max_share=1), dict(max_share=100, weight="flat"),
           dict(max_gap=1), dict(min_shared=2), dict(min_score=1_000_000),
           dict(max_share=100, min_words=5, max_gap=1, min_works=3, weight="rarity")]


@pytest.mark.parametrize("kw", OPTIONS, ids=lambda kw: "-".join(
    "%s_%s" % (k, v) for k, v in kw.items()) or "defaults")
@pytest.mark.parametrize("n_active", [1, 2, 63, 64, 65, 257])
def test_random_fandoms_with_planted_families(n_active, kw):
    rng = np.random.default_rng(1000 + n_active)
    cols, same, n_works, n_spell = fandom(rng, n_active)
    works, found, pairs = check(cols, same, n_works, n_spell, **kw)
    short = kw.get("min_words", 6) <= 5                       # the run of five is a passage
    assert int((works["passage_records"] > 0).sum()) == n_active + short
    if kw.get("max_share") == 1 or kw.get("min_score", 1) > 1000 or n_active + short == 1:
        assert len(pairs) == 0 and not works["partners"].any()
    if kw.get("max_share") == 1:
        assert not found["telling"].any() and not works["telling"].any()
    elif n_active >= 63 and "min_shared" not in kw and "min_score" not in kw:
        assert len(pairs) > 10 and len(found) > 10
        assert (found["telling"] == 0).any() == ("max_share" not in kw)


def test_no_records_and_one_record():
    none = [np.zeros(0, dtype=np.uint32)] * 4
    works, found, pairs = check(none, script_same(3), 2, 3)
    assert works.tolist() == [(0, 0, 0, 0, 0, 0, NONE, 0)] * 2 and not len(found) and not len(pairs)
    one = [np.asarray([v], dtype=np.uint32) for v in (1, 9, 2, 6)]
    works, found, pairs = check(one, script_same(3), 3, 7, min_words=1)
    assert works["passage_records"].tolist() == [0, 1, 0] and works["singular"].tolist() == [0, 1, 0]
    assert check(one, script_same(3), 3, 7)[0]["passage_records"].tolist() == [0, 0, 0]


def test_posting_lists_of_every_rank_path():
    """Lists of 2 to 257 works in one input: a list of more than 64 works is ranked by a wave,
    and the contributions of one list cross wave and workgroup edges of the expansion."""
    sizes = (2, 3, 63, 64, 65, 66, 257)
    n = 300
    quotes = [(w, 10, verbatim(10, **{"w%d" % j: WRONG + j for j, k in enumerate(sizes)
                                      if (w * 7) % n < k})) for w in range(n)]
    works, found, pairs = check(layout(quotes), script_same(40), n, WRONG + 10, max_share=100)
    assert sorted(found["works"].tolist()) == list(sizes) and found["telling"].all()
    assert len(pairs) == 257 * 256 // 2 and int(works["partners"].max()) == 256
    assert int(pairs["shared"].max()) == len(sizes)


def test_one_list_of_2049_works_against_the_closed_form():
    """2 098 176 contributions: past where a 32-bit float's square root unranks the triangle
    exactly.  Every pair once, in (a, b) order, shared 1 and one score."""
    n = 2049
    quotes = [(w, 10, verbatim(10, 6, w2=WRONG)) for w in range(n)]
    cols = layout(quotes)
    works, found, pairs = misquotes.find_misquotes(*cols, script_same(20), n, WRONG + 1,
                                                   max_share=100)
    assert found.tolist() == [(12, WRONG, n, n, n, 1, 1, 0)]
    a, b = np.triu_indices(n, 1)
    assert len(pairs) == n * (n - 1) // 2 == 2_098_176
    assert (pairs["a"] == a).all() and (pairs["b"] == b).all()
    for name, value in (("shared", 1), ("score", 1), ("a_on_common", 1), ("b_on_common", 1),
                        ("strongest", 0), ("strongest_weight", 1)):
        assert (pairs[name] == value).all(), name
    assert (works["partners"] == n - 1).all() and (works["closest_score"] == 1).all()
    assert works["closest"].tolist() == [1] + [0] * (n - 1)
    assert (works["telling"] == 1).all() and (works["passage_records"] == 6).all()


@pytest.mark.parametrize("n_works", [48 * 1024 * 8, 48 * 1024 * 8 + 1])
def test_long_rows_where_a_bit_per_work_fits_the_lds_and_where_it_does_not(n_works):
    """70 works spread over all work numbers share one misquote: rows of up to 69 partners, placed
    by a bit per work in LDS at 393 216 works and by comparisons one work past that."""
    ids = np.linspace(0, n_works - 1, 70).astype(np.int64)
    quotes = [(int(w), 10, verbatim(10, 6, w2=WRONG)) for w in ids]
    works, found, pairs = misquotes.find_misquotes(*layout(quotes), script_same(20), n_works,
                                                   WRONG + 1, max_share=100)
    a, b = np.triu_indices(70, 1)
    assert found.tolist() == [(12, WRONG, 70, 70, 70, 1, 1, 0)]
    assert pairs["a"].tolist() == ids[a].tolist() and pairs["b"].tolist() == ids[b].tolist()
    assert (pairs["shared"] == 1).all() and (pairs["strongest"] == 0).all()
    assert works["partners"][ids].tolist() == [69] * 70 and int(works["partners"].sum()) == 69 * 70
    assert works["closest"][ids].tolist() == [int(ids[1])] + [0] * 69


def test_two_works_sharing_300_misquotes():
    """Three hundred contributions to one pair slot; the strongest is the first of the 150 that
    tie on the larger weight."""
    quotes = []
    for w in (0, 1):
        quotes += [(w, 10 * l, [WRONG + 6 * l + k for k in range(6)]) for l in range(50)]
    quotes += [(w, 10 * l, verbatim(10 * l, 6)) for w in range(2, 8) for l in range(25, 50)]
    same = np.arange(510, dtype=np.uint32)
    works, found, pairs = check(layout(quotes), same, 8, WRONG + 300, max_share=100)
    assert pairs.tolist() == [(0, 1, 300, 150 + 150 * 3, 300, 300, 150, 3)]
    assert found["weight"].tolist() == [1] * 150 + [3] * 150


@pytest.mark.parametrize("bits", ["4", "0"])
@pytest.mark.parametrize("kw", [dict(), dict(max_share=100, max_gap=1, min_words=5)],
                         ids=["defaults", "share100"])
def test_hash_bits_change_nothing(monkeypatch, bits, kw):
    monkeypatch.setenv("FS_MISQUOTES_HASH_BITS", bits)
    cols, same, n_works, n_spell = fandom(np.random.default_rng(7), 60)
    assert len(cols[0]) <= 2000
    _, found, pairs = check(cols, same, n_works, n_spell, **kw)
    assert len(found) > 5 and len(pairs) > 5


# ---- capacity, the bound and the refusals ----------------------------------------------------

def call(cols, same, n_works, n_spell, cap_m, cap_p, n_script=None, min_words=6, max_gap=0,
         min_works=2, max_share=50, weight=0, min_shared=1, min_score=1):
    L = _lib.load()
    works = np.full(n_works, 9, dtype=np.uint32).repeat(8).view(abi.MISQUOTE_WORK_DTYPE)
    found = np.zeros(max(cap_m, 1), dtype=abi.MISQUOTE_DTYPE)
    pairs = np.zeros(max(cap_p, 1), dtype=abi.MISQUOTE_PAIR_DTYPE)
    got = [C.c_uint64(99), C.c_uint64(99)]
    rc = L.fs_misquotes(0, *(abi.ptr(c, C.c_uint32) for c in cols), abi.ptr(same, C.c_uint32),
                        len(cols[0]), n_works, len(same) if n_script is None else n_script,
                        n_spell, min_words, max_gap, min_works, max_share, weight, min_shared,
                        min_score, works.ctypes.data_as(C.c_void_p),
                        found.ctypes.data_as(C.c_void_p) if cap_m else None, cap_m,
                        C.byref(got[0]), pairs.ctypes.data_as(C.c_void_p) if cap_p else None,
                        cap_p, C.byref(got[1]))
    return rc, [g.value for g in got], works, found, pairs


def small():
    cols, same, n_works, n_spell = fandom(np.random.default_rng(11), 20)
    want = mr.misquotes(list(zip(*(c.tolist() for c in cols))), same.tolist(), n_works, n_spell)
    return cols, same, n_works, n_spell, want


def test_caps_give_the_counts_and_a_complete_works_table():
    cols, same, n_works, n_spell, (want_w, want_m, want_p) = small()
    n_m, n_p = len(want_m), len(want_p)
    assert n_m > 3 and n_p > 3
    for cap_m, cap_p in ((0, 0), (n_m - 1, n_p), (n_m, n_p - 1), (n_m, n_p), (n_m + 5, n_p + 5)):
        rc, got, works, found, pairs = call(cols, same, n_works, n_spell, cap_m, cap_p)
        fits = cap_m >= n_m and cap_p >= n_p
        assert rc == (abi.FS_OK if fits else abi.FS_E_CAPACITY) and got == [n_m, n_p]
        for name in mr.WORK_KEYS:
            assert works[name].tolist() == [d[name] for d in want_w], name
        if fits:
            assert found[:n_m]["spell"].tolist() == [d["spell"] for d in want_m]
            assert pairs[:n_p]["score"].tolist() == [d["score"] for d in want_p]
        else:
            assert not found["works"].any() and not pairs["shared"].any()
    ms = (C.c_double * 8)()
    assert _lib.load().fs_misquotes_times(ms) == abi.FS_OK and all(t > 0 for t in ms)


def test_max_pairs_refuses_at_eleven_contributions(monkeypatch):
    monkeypatch.setenv("FS_MISQUOTES_MAX_PAIRS", "10")
    ten = [(w, 10, verbatim(10, 6, w1=WRONG)) for w in range(5)] + \
        [(w, 10, verbatim(10, 6)) for w in range(5, 12)]
    cols = layout(ten)
    rc, got, _, _, _ = call(cols, script_same(30), 12, WRONG + 2, 50, 50)
    assert rc == abi.FS_OK and got == [1, 10]
    eleven = ten[:10] + [(w, 10, verbatim(10, 6, w4=WRONG + 1)) for w in (10, 11)]
    rc, got, _, _, _ = call(layout(eleven), script_same(30), 12, WRONG + 2, 50, 50)
    assert rc == abi.FS_E_UNSUPPORTED
    err = _lib.load().fs_last_error()
    assert b"P = 11" in err and b"--max-share" in err
    monkeypatch.setenv("FS_MISQUOTES_MAX_PAIRS", "11")
    assert call(layout(eleven), script_same(30), 12, WRONG + 2, 50, 50)[:2] == (abi.FS_OK, [2, 11])


def test_every_invalid_input():
    cols, same, n_works, n_spell, _ = small()
    L = _lib.load()
    ok = dict(cap_m=500, cap_p=5000)
    assert call(cols, same, n_works, n_spell, **ok)[0] == abi.FS_OK
    swapped = [c.copy() for c in cols]
    for c in swapped:
        c[[3, 4]] = c[[4, 3]]
    assert call(swapped, same, n_works, n_spell, **ok)[0] == abi.FS_E_INVALID
    assert b"sorted" in L.fs_last_error()
    assert call([c[::-1].copy() for c in cols], same, n_works, n_spell, **ok)[0] == abi.FS_E_INVALID
    assert call(cols, same, int(cols[0].max()), n_spell, **ok)[0] == abi.FS_E_INVALID
    assert call(cols, same, n_works, n_spell, n_script=int(cols[2].max()), **ok)[0] == abi.FS_E_INVALID
    assert call(cols, same, n_works, int(cols[3].max()) + 1, **ok)[0] == abi.FS_OK
    assert call(cols, same, n_works, int(cols[3].max()), **ok)[0] == abi.FS_E_INVALID
    assert b"n_spell" in L.fs_last_error()
    bad_same = same.copy()
    bad_same[len(same) - 1] = n_spell                         # a word without a record
    assert call(cols, bad_same, n_works, n_spell, **ok)[0] == abi.FS_E_INVALID
    assert b"same" in L.fs_last_error()
    bad_same[len(same) - 1] = n_spell - 1
    assert call(cols, bad_same, n_works, n_spell, **ok)[0] == abi.FS_OK
    for bad in (dict(min_words=0), dict(min_works=1), dict(max_share=0), dict(max_share=101),
                dict(weight=2), dict(min_shared=0), dict(min_score=0)):
        assert call(cols, same, n_works, n_spell, **ok, **bad)[0] == abi.FS_E_INVALID, bad
    assert call(cols, same, n_works, n_spell, n_script=(1 << 19) + 1, **ok)[0] == abi.FS_E_UNSUPPORTED


def test_against_fs_variants_when_every_record_is_in_a_passage():
    cols, same, n_works, n_spell = fandom(np.random.default_rng(5), 120)
    kw = dict(min_words=1, max_gap=0, min_works=2, max_share=100)
    works, found, _ = check(cols, same, n_works, n_spell, **kw)
    assert int(works["passage_records"].sum()) == len(cols[0])
    _, cells = variants.find_variants(cols[0], cols[2], cols[3], n_works, len(same), n_spell)
    cell = {(c[0], c[1]): (c[2], c[3]) for c in cells.tolist()}
    assert len(found) > 20
    for o, s, records, k in found[["orig_ix", "spell", "records", "works"]].tolist():
        assert cell[o, s] == (records, k) and s != same[o] and k >= 2
    listed = {(o, s) for o, s in found[["orig_ix", "spell"]].tolist()}
    assert listed == {key for key, (_, k) in cell.items() if k >= 2 and key[1] != same[key[0]]}


# ---- the command -----------------------------------------------------------------------------

def run_both(tmp_path, path, extra=(), tag="m"):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (tag, reader)))
        assert main(["misquotes", path, "-o", prefix, "--reader", reader, *extra]) == 0
        got[reader] = tuple(open(name, "rb").read()
                            for name in misquotes.output_names(path, prefix))
    assert got["device"] == got["python"]
    return got["device"]


@pytest.mark.parametrize("case,options,kw", mmg.CASES)
def test_golden_cases_under_both_readers(tmp_path, case, options, kw):
    out = run_both(tmp_path, os.path.join(GOLDEN, mmg.INPUT), options)
    for name, part in zip(mmg.golden_names(case), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_a_file_without_records_and_a_file_with_one_active_work(tmp_path):
    from tests.passages_restated import MATCH_FIELDS
    heads = tuple((",".join(f) + "\r\n").encode() for f in
                  (mr.MISQUOTE_FIELDS, mr.PAIR_FIELDS, mr.WORK_FIELDS))
    empty = tmp_path / "empty.csv"
    empty.write_bytes((",".join(MATCH_FIELDS) + "\r\n").encode())
    assert run_both(tmp_path, str(empty), tag="e") == heads
    with open(os.path.join(GOLDEN, mmg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    one = tmp_path / "one.csv"
    one.write_bytes(b"\r\n".join(l for l in lines if l.startswith((b"FAN_", b"a.txt,"))) + b"\r\n")
    out = run_both(tmp_path, str(one), tag="o")
    assert out[1] == heads[1] and out[0] == heads[0] and out[2].count(b"\r\n") == 2
    assert out == tuple(p.encode("utf-8") for p in mr.misquotes_csv(one.read_bytes().decode("utf-8")))


def test_two_labels_for_one_script_word(tmp_path):
    with open(os.path.join(GOLDEN, mmg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    parts = lines[33].split(b",")
    parts[-4] = b"99"                             # the same script word in another scene
    lines[33] = b",".join(parts)
    path = tmp_path / "m.csv"
    path.write_bytes(b"\r\n".join(lines))
    errs = []
    for reader in ("device", "python"):
        with pytest.raises(SystemExit) as e:
            main(["misquotes", str(path), "-o", str(tmp_path / "o"), "--reader", reader])
        errs.append(str(e.value.code))
    assert errs[0] == errs[1]
    assert errs[0].startswith("ao3.py misquotes: error: script word ") and "two scenes" in errs[0]
