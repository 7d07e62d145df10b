"""The harness of tests/test_gpu_levenshtein.py, pinned without a GPU: the plain DP against the
restated reference and known answers, the predicted records against the C oracle, and a census
of the edges the case lists must contain."""

import itertools

import numpy as np
import pytest

from oracle import search_restated as sr
from tests import levpairs as lp


def _operands(name):
    n, pairs = lp.cases(name)
    return n, [(p, lp.script_text(p), lp.fan_text(p)) for p in pairs]


def test_distance_known_answers():
    """The answers of test_oracle_known_answers.py, by all three formulations."""
    known = [("kitten", "sitting", 3), ("", "abc", 3), ("flaw", "lawn", 2),
             ("Hello world!", "Holly grail!", 7), ("Brian", "Jesus", 5), ("Saturday", "Sunday", 3),
             ("intention", "execution", 5), ("gumbo", "gambol", 2), ("été", "ete", 2),
             ("", "", 0), ("a", "", 1)]
    for n in (2, 4, 6, 10):
        ws = ["w%d" % i for i in range(n)]
        known.append((" ".join(ws), "[" + ", ".join(ws) + "]", n + 1))
    for a, b, d in known:
        for f in (lp.distance, lp.distance_plain, lp.distance_rows, sr.lev_distance):
            assert f(a, b) == d and f(b, a) == d, (f.__name__, a, b)


@pytest.mark.parametrize("name", lp.ALL_LISTS + lp.LIMIT_LISTS)
def test_rows_formulation_equals_plain_dp(name):
    """The numpy rows equal the plain DP on every case under 130 code points, and on the first
    large cases of every list."""
    n, ops = _operands(name)
    large = 0
    for p, a, b in ops:
        if len(a) < lp.PLAIN_BELOW and len(b) < lp.PLAIN_BELOW:
            assert lp.distance_rows(a, b) == lp.distance(a, b) == lp.pair_distance(p), p.name
        elif large < 3:
            large += 1
            assert lp.distance_plain(a, b) == lp.distance(a, b), p.name


@pytest.mark.parametrize("name", ("sub4", "sub16", "sub6_a", "sub6_b", "words6", "words6_long", "grid6_rand2")
                         + lp.ALPHA_LISTS)
def test_distance_equals_restated_reference(name):
    """levpairs.distance against oracle.search_restated.lev_distance on a sample of the
    generators' output: some of the lists; of those every case of the short ones, every seventh
    of the long ones, and only the first four large cases of each (the restated reference is
    plain Python too).  Every case of every list meets the C oracle's own DP in
    test_oracle_rows_are_the_predicted_ones."""
    n, ops = _operands(name)
    step = 1 if len(ops) < 140 else 7
    large = 0
    for p, a, b in ops[::step]:
        if max(len(a), len(b)) >= 200:
            large += 1
            if large > 4:
                continue
        assert lp.distance(a, b) == sr.lev_distance(a, b), p.name


@pytest.mark.parametrize("layout", ("own", "vec"))
@pytest.mark.parametrize("name", lp.ALL_LISTS + lp.LIMIT_LISTS)
def test_oracle_rows_are_the_predicted_ones(name, layout):
    """Count, work, fan_ix, orig_ix and lev of the C oracle's rows for every case list the GPU
    tests use, in both string-id layouts (tok_str == tok passed explicitly gives the rows of
    "vec": checked on one list)."""
    b, want = lp.oracle_rows(name, layout)
    lp.assert_predicted(want, b)
    assert len(want) == b.n * sum(not p.name.startswith(lp.UNQUOTED) for p in b.pairs)
    # every script n-gram unique, one window per quoted work
    assert len(set(b.script.tolist())) == len(b.script) == b.n * len(b.pairs)
    assert set(np.diff(b.off).tolist()) <= {0, b.n}


def test_explicit_string_ids_give_the_same_oracle_rows():
    b, want = lp.oracle_rows("words6", "vec")
    bx = lp.build(lp.cases("words6")[1], 6, "vec_explicit")
    assert bx.tok_str is not None and (bx.tok_str == bx.tok).all() and b.tok_str is None
    from fandom_search_amd import abi
    got = lp.oracle_search(bx, abi.make_config(window_size=6))
    assert got.tobytes() == want.tobytes()


def test_split():
    rng = np.random.default_rng(0)
    for total, n, how in itertools.product((0, 1, 5, 64, 507), (1, 2, 6, 16), lp.SPLITS):
        ls = lp.split(total, n, how, rng)
        assert len(ls) == n and sum(ls) == total and min(ls) >= 0
    assert lp.split(7, 3, "first") == [7, 0, 0] and lp.split(7, 3, "last") == [0, 0, 7]
    assert lp.split(7, 3, "even") == [3, 2, 2]


# ---- census: the edges are really in the lists ---------------------------------------------

def _wave_pattern_length(la, lb):
    """lev_wave's rule: the longer operand when both fit in 64, otherwise the one that fits
    (the shorter); over 64 means the scratch DP."""
    return max(la, lb) if la <= 64 and lb <= 64 else min(la, lb)


def _cells(ops, kind=None):
    return {(len(a), len(b)) for p, a, b in ops if kind is None or p.name.startswith(kind + " ")}


def test_census_length_grid():
    full = set(itertools.product(lp.la_grid(6), lp.lb_grid(6)))
    assert len(full) == 13 * 17
    sub = {c for c in full if max(c) <= lp.SUB_MAX}
    seen_kinds = set()
    for kind in lp.BIG_CONTENTS:
        n, ops = _operands("grid6_" + kind)
        assert n == 6 and _cells(ops, kind) == full
        seen_kinds.add(kind)
    for name in ("sub6_a", "sub6_b"):
        n, ops = _operands(name)
        kinds = {p.name.split(" ")[0] for p, a, b in ops}
        for kind in kinds:
            assert _cells(ops, kind) == sub, (name, kind)
        seen_kinds |= kinds
    assert seen_kinds == set(lp.CONTENTS)
    # the splits over the words vary on both sides, zero-length words included
    for name in lp.GRID_LISTS:
        n, ops = _operands(name)
        hows = {p.name.rsplit(" ", 1)[1] for p, a, b in ops}
        assert {h.split("/")[0] for h in hows} == set(lp.SPLITS) == {h.split("/")[1] for h in hows}
        assert any("" in p.swords for p, a, b in ops) and any("" in p.fwords for p, a, b in ops)


def test_census_myers_edges():
    """What the length grid is for, computed from the built operands of every grid list."""
    for name in lp.GRID_LISTS:
        n, ops = _operands(name)
        cells = _cells(ops)
        m = {_wave_pattern_length(la, lb) for la, lb in cells}
        assert {31, 32, 33, 63, 64} <= m, name                   # the score bit at 31/32 and 63/64
        assert any(la == lb for la, lb in cells)
        assert any(la <= 64 < lb for la, lb in cells) and any(lb <= 64 < la for la, lb in cells)
        assert any(la > 64 and lb > 64 for la, lb in cells)       # scratch DP
        assert any(la >= lb and lb <= 64 and la <= 64 for la, lb in cells)      # script as pattern
        assert any(la < lb <= 64 for la, lb in cells)             # fan text as pattern
        # the text (the other operand) ends on, one before and one past a 64-column block
        t = {(min(la, lb) if la <= 64 and lb <= 64 else max(la, lb)) % 64 for la, lb in cells
             if _wave_pattern_length(la, lb) <= 64}
        assert {0, 1, 63} <= t, name
        # the lane paths: pattern = script window of 32, 33, 64 code points, 65 hands over
        assert {31, 32, 33, 63, 64, 65} <= {la for la, lb in cells}
    for kind in lp.BIG_CONTENTS:
        cells = _cells(_operands("grid6_" + kind)[1])
        assert (512, 512) in cells and (5, 512) in cells and (512, 12) in cells and (64, 512) in cells


def test_census_contents():
    n, ops = _operands("sub6_b")
    foreign = [(a, b) for p, a, b in ops if p.name.startswith("foreign ")]
    script_alphabet = set("".join(a for a, b in foreign))
    for ch in lp.FOREIGN:
        assert any(ch in b for a, b in foreign) and ch not in script_alphabet
    assert ord(lp.FOREIGN[2]) > 0xFFFF and 0x4E00 <= ord(lp.FOREIGN[1]) <= 0x9FFF
    punct = "".join(a for p, a, b in ops if p.name.startswith("punct "))
    assert {"[", ",", "]"} <= set(punct)
    n, ops = _operands("sub6_a")
    for p, a, b in ops:
        if p.name.startswith("repeat "):
            assert set(a) <= {"a", " "} and set(b) <= set("a[], ")
        if p.name.startswith("period2 ") and len(a) > 20 and len(b) > 20:
            assert "abab" in a.replace(" ", "") and "baba" in b.replace(", ", "")
    # long carry chains: two-letter texts have long runs of equal characters against each other
    n, ops = _operands("grid6_rand2")
    assert all(set(a) <= set("ab ") for p, a, b in ops if p.name != "spacer")
    # the shifted copy: first character dropped
    n, ops = _operands("grid6_shifted")
    hit = 0
    for p, a, b in ops:
        wa, wb = "".join(p.swords), "".join(p.fwords)
        if len(wa) > 3 and len(wb) >= len(wa):
            assert wb.startswith(wa[1:])
            hit += 1
    assert hit > 50


@pytest.mark.parametrize("n", lp.WINDOW_SIZES)
def test_census_window_sizes(n):
    nn, ops = _operands("sub%d" % n)
    assert nn == n
    want = {(la, lb) for la in lp.la_grid(n) for lb in lp.lb_grid(n) if max(la, lb) <= lp.SUB_MAX}
    assert _cells(ops) == want and len(want) > 90
    assert {p.name.split(" ")[0] for p, a, b in ops} == set(lp.CONTENTS)
    if n == 1:
        assert any(a == "" for p, a, b in ops)                   # la = 0
    if n == 16:
        assert min(len(b) for p, a, b in ops) >= 32
        assert any(all(len(w) > 0 for w in p.fwords) for p, a, b in ops)


def test_census_fan_word_lengths():
    n, ops = _operands("words6")
    for slot in (0, 3, 5):
        assert {len(p.fwords[slot]) for p, a, b in ops} >= set(lp.FAN_WORD_LENGTHS), slot
    assert max(len(b) for p, a, b in ops) <= 512 and max(len(a) for p, a, b in ops) <= 64
    # at 15 and 16 the 15th and 16th characters decide the distance
    for L, at in ((15, 14), (16, 14), (16, 15)):
        decided = False
        by_rest = {}
        for p, a, b in ops:
            for slot in (0, 3, 5):
                w = p.fwords[slot]
                if len(w) == L:
                    key = (slot, p.swords, w[:at] + w[at + 1:])
                    by_rest.setdefault(key, set()).add((w[at], lp.pair_distance(p)))
        for vals in by_rest.values():
            if len({d for ch, d in vals}) > 1:
                decided = True
        assert decided, (L, at)
    n, ops = _operands("words6_long")
    assert all(len(a) <= 64 for p, a, b in ops) and sum(len(b) > 512 for p, a, b in ops) >= 12
    assert {255, 256, 257, 254, 300, 16, 15} <= {len(w) for p, a, b in ops for w in p.fwords}


def test_census_alphabets_and_limits():
    for size in lp.ALPHABET_SIZES:
        n, pairs = lp.cases("alpha%d" % size)
        assert lp.alphabet_size(pairs) == size
        b = lp.build(pairs, n, "own")
        assert len(set(" ".join(b.swords))) == size               # as fs_index_create counts it
        assert any(ch in w for p in pairs for w in p.fwords for ch in lp.FOREIGN)
    for want in (1023, 1024):
        n, pairs = lp.cases("limit_d%d" % want)
        assert [lp.pair_distance(p) for p in pairs].count(want) == 1
        assert all(len(lp.script_text(p)) <= 64 for p in pairs)
    for name in ("limit_la513_unquoted", "limit_la513_quoted"):
        n, pairs = lp.cases(name)
        long_ones = [p for p in pairs if len(lp.script_text(p)) == 513]
        assert len(long_ones) == 1 and max(len(lp.script_text(p)) for p in pairs) == 513
        assert long_ones[0].name.startswith(lp.UNQUOTED) == name.endswith("unquoted")
        b = lp.build(pairs, n, "own")
        assert (len(b.tok) < len(b.script)) == name.endswith("unquoted")
    n, pairs = lp.cases("limit_lb513")
    assert max(len(lp.fan_text(p)) for p in pairs) == 513 and all(len(lp.script_text(p)) <= 64 for p in pairs)


def test_spacers_keep_straddling_windows_within_512():
    """String id == vector id: every script window, quoted or not, stays within 512 code points
    on both sides in the lists that the table paths must take whole."""
    for name in lp.WAVE_SAFE_LISTS:
        n, pairs = lp.cases(name)
        b = lp.build(pairs, n, "vec")
        sl = np.array([len(w) for w in b.swords])
        fl = np.array([len(w) for p in b.pairs for w in p.fwords])
        cs, cf = np.concatenate([[0], np.cumsum(sl)]), np.concatenate([[0], np.cumsum(fl)])
        assert (cs[n:] - cs[:-n]).max() + n - 1 <= 512, name
        assert (cf[n:] - cf[:-n]).max() + 2 * n <= 512, name
