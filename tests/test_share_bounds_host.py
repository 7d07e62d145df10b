"""The share rule's arithmetic on window pairs built at its bounds (tests/share_restated.py), on the
CPU: which pairs are records is decided in exact integer arithmetic on the float32 table entries
(every entry times 2^60 is an integer; cos > 1 - thr as a comparison of squares), and on every
record the restated rule must ask for a mask inside the agreeing set and pass the pairs' test --
soundness at the bound, for windows of six to twelve slots under three (thr, gamma).  Closeness is
a condition here, not a measurement: per family the closest record lies within 2e-3 of phi and, in
the run at its bound, within 2e-3 of the integer threshold (share_restated's docstring has the
figures).  test_gpu_share_bounds.py runs the kernels on the same pairs."""

import itertools
import math

import numpy as np
import pytest

from tests import share_restated as sr

# the runs as fs_hash.h's comment gives them: 7 = 4 + 3, 9 = 5 + 4, 11 = 4 + 4 + 3
RUNS = {6: (6,), 7: (4, 3), 8: (4, 4), 9: (5, 4), 10: (5, 5), 11: (4, 4, 3), 12: (4, 4, 4)}
CLOSE = 2e-3


@pytest.fixture(scope="module", params=[(n, c) for n in sr.SIZES for c in range(len(sr.CONFIGS))],
                ids=lambda p: "n%d-thr%g-gamma%g" % ((p[0],) + sr.CONFIGS[p[1]]))
def built(request):
    n, c = request.param
    return sr.Bounds(n, *sr.CONFIGS[c])


def bound_run(b, pair, qi, wild, far):
    """(agreeing integer sum - threshold) / threshold in the runs that hold far slots next to
    agreeing ones: the smallest that is not negative, or None."""
    best = None
    for k0, k1 in b.runs:
        mine = [k for k in range(k0, k1) if far >> k & 1]
        agree = [k for k in range(k0, k1) if not far >> k & 1 and not wild[k]]
        if not mine or not agree:
            continue
        thr = b.rule.run_threshold(qi, wild, k0, k1)
        x = (sum(qi[k] for k in agree) - thr) / thr
        if x >= 0 and (best is None or x < best):
            best = x
    return best


def test_the_table_is_what_the_pairs_need(built):
    b = built
    ex = sr.Exact(b)
    rows = lambda prefix: [r for key, r in b.row_id.items() if isinstance(key, tuple) and key[0] == prefix]
    for t, d in enumerate(sr.TWINS):               # far, under what k_near_pairs takes for near in float32
        for u in rows("u%d" % t)[:4]:
            for v in rows("v%d" % t)[:4]:
                c = ex.cosine(u, v)
                assert abs(c - (b.gamma - d)) < 2e-6 and c < b.gamma - 1e-4 - 1e-5
    for t in range(2):
        c = ex.cosine(rows("nu%d" % t)[0], rows("nv%d" % t)[0])
        assert abs(c - (b.gamma + sr.NEAR)) < 2e-6
    # directions are orthogonal but for the twins; rows of one direction are parallel
    reps = {}
    for key, r in b.row_id.items():
        if isinstance(key, tuple):
            reps.setdefault(key[0], r)
    for (da, ra), (db, rb) in itertools.combinations(sorted(reps.items()), 2):
        twin = da.lstrip("nuv") == db.lstrip("nuv") and da[:1] in "nuv" and db[:1] in "nuv" and not da.startswith("g")
        if not twin:
            assert ex.dot(ra, rb) == 0, (da, db)
    g = rows("g0")
    assert len(g) > 2 and all(ex.dot(g[0], r) ** 2 == ex.dot(g[0], g[0]) * ex.dot(r, r) for r in g)
    # out-of-vocabulary fan tokens are provably far from every row (fs_build_share: oov_far)
    kappa = max(float(abs(v).max()) / math.sqrt(b.q[r]) for r, v in enumerate(b.emb) if b.q[r] > 0)
    assert math.sqrt(3.0) * kappa * (1.0 + 1e-5) <= b.gamma - 1e-4
    assert sum(1 for x in b.q if x == 0.0) == 2 and 200 <= len(b.emb) <= 900
    sizes = b.component_sizes()
    assert sum(sizes) == len(b.emb) and sizes.count(1) >= 2


def test_the_texts_place_the_windows_where_kernels_go_wrong(built):
    b = built
    n = b.n
    starts = [p.stream_at % 256 for p in b.pairs]
    assert any(256 - n < s for s in starts) and any(250 <= s for s in starts)     # across a sub-tile's seam
    assert b.pairs[-1].stream_at + n == len(b.tok)                                  # the stream's last window
    assert any(int(b.off[p.work + 1]) == p.stream_at + n for p in b.pairs if p.work + 2 < len(b.off))   # ends a work
    assert all(p.f_at != p.s_at and p.stream_at != p.s_at for p in b.pairs)
    assert 2 <= len(b.off) - 1 <= 4
    for p in b.pairs:
        assert list(b.tok[p.stream_at:p.stream_at + n]) == p.fan and list(b.script[p.s_at:p.s_at + n]) == p.script
        assert int(b.off[p.work]) + p.f_at == p.stream_at


@pytest.mark.parametrize("all_wild", [False, True])
def test_the_rule_is_sound_on_every_record_at_the_bound(built, all_wild):
    """all_wild: the index built with FS_LSH_SHARE=43, where every fan name agrees with anything."""
    b = built
    ex, rule, n = sr.Exact(b), b.rule, b.n
    assert [k1 - k0 for k0, k1 in sr.runs_of(n)] == list(RUNS[n])
    starts = list(itertools.accumulate((0,) + RUNS[n]))
    records = 0
    for pair in b.pairs:
        qi, wild, usable, q = b.window(pair.fan, all_wild)
        masks = rule.asks(qi, wild, usable, n)
        far = b.far_mask(pair, all_wild)
        ladder = sr.family_of(pair) not in ("wild_large", "all_wild", "cap")
        if ladder:
            assert masks is not None, pair            # (the rule is on its way: not around it)
        if masks is not None:
            for m in masks:
                # a mask: slots of one run, usable, and heavy there however the sum is made
                r = max(i for i, s in enumerate(starts[:-1]) if m >> s)
                ks = [k for k in range(n) if m >> k & 1]
                assert m and all(starts[r] <= k < starts[r + 1] for k in ks) and all(usable[k] for k in ks), (pair, m)
                run = range(starts[r], starts[r + 1])
                need = float(rule.lim) * sum(q[k] for k in run) - sum(q[k] for k in run if wild[k]) - (len(run) + 4) / rule.scale
                assert sum(q[k] for k in ks) >= need * (1 - 1e-6), (pair, m)
        if not ex.is_record(pair):
            continue
        records += 1
        agree = ~far & ((1 << n) - 1)
        assert masks is None or any(m & ~agree == 0 for m in masks), (pair, "no mask inside the agreeing set")
        assert rule.pair_possible(far, q, [b.q_of(s) for s in pair.script]), (pair, "the pairs' test")
    assert records > len(b.pairs) // 5


def test_every_family_reaches_the_bound(built):
    b = built
    ex, rule, n = sr.Exact(b), b.rule, b.n
    fams = {}
    for pair in b.pairs:
        fams.setdefault(sr.family_of(pair), []).append(pair)
    want = {"pos", "in_run", "wild2", "name3", "zero_agree", "zero_far", "wild_large", "all_wild", "cap"}
    want |= {"two_runs", "all_of_run"} if n >= 7 else set()
    want |= {"every_run"} if n >= 11 else set()
    assert set(fams) == want
    for fam, pairs in sorted(fams.items()):
        if fam in ("wild_large", "all_wild", "cap"):
            continue
        best = None
        for pair in pairs:
            qi, wild, usable, q = b.window(pair.fan)
            far = b.far_mask(pair)
            A = sum(q[k] for k in range(n) if far >> k & 1) / sum(q)
            rec = ex.is_record(pair)
            if pair.delta >= 1e-2:
                assert rec, pair                      # inside
            if pair.delta <= -1e-3:                   # outside: the pairs' test leaves at once
                assert not rec and A >= rule.phi * (1 + 1e-9) and not rule.pair_possible(far, q, [b.q_of(s) for s in pair.script]), pair
            if rec and pair.twin == 0:
                x = ((rule.phi - A) / rule.phi, bound_run(b, pair, qi, wild, far))
                # (closest among the records whose far run is at its own bound as well)
                if (x[1] is not None or fam == "all_of_run") and (best is None or x[0] < best[0]):
                    best = x
        assert best is not None and 0 < best[0] <= CLOSE, (fam, best)
        if fam != "all_of_run":                       # (its far run has no agreeing slot: module docstring)
            assert best[1] is not None and best[1] <= CLOSE, (fam, best)
        print("%-12s n=%2d thr=%.2f gamma=%.2f  (phi - A) / phi = %.2e  (sum - thr) / thr = %s"
              % (fam, n, b.thr, b.gamma, best[0], "%.2e" % best[1] if best[1] is not None else "-"))


def test_the_special_windows_are_what_they_are_called(built):
    b = built
    rule, n = b.rule, b.n
    for pair in b.pairs:
        fam = sr.family_of(pair)
        qi, wild, usable, q = b.window(pair.fan, all_wild=not b.script_names)
        masks = rule.asks(qi, wild, usable, n)
        if fam == "wild_large":
            k = wild.index(True)
            assert qi[k] == max(qi) and masks is None
        if fam == "all_wild":
            r = int(pair.family.rsplit("_", 1)[1])
            assert all(wild[k] for k in range(*b.runs[r])) and masks is None
        if fam == "wild2":
            assert sum(wild) == 1 and 0 < qi[wild.index(True)] < min(x for x, w in zip(qi, wild) if not w and x) and masks
        if fam == "cap":
            count = {(6, 0.5): 20, (10, 0.5): 20}.get((n, b.gamma))
            assert masks is not None and (count is None or len(masks) == count == sr.K_ENUM_CAP)
    assert b.unconstrained_windows(all_wild=not b.script_names) >= 1 + len(b.runs)


def test_no_window_of_up_to_twelve_slots_asks_for_more_than_the_cap():
    """An antichain per run: C(6, 3) = 20, C(5, 2) + C(5, 2) = 20, 3 C(4, 2) = 18.  The kernel's
    `cnt > cap` outcome is restated, and is unreachable at kEnumCap = 20."""
    rng = np.random.default_rng(11)
    top = 0
    for n in sr.SIZES:
        for thr, gamma in sr.CONFIGS:
            rule = sr.Rule(thr, gamma, 8.0)
            for trial in range(150):
                q = rng.lognormal(np.log(30.0), [0.02, 0.3, 1.0][trial % 3], size=n)
                qi = rule.shares(q)
                got = rule.asks(qi, [False] * n, [True] * n, n, cap=10 ** 6)
                if got is not None:
                    assert len(got) <= sr.K_ENUM_CAP
                    top = max(top, len(got))
                    assert rule.asks(qi, [False] * n, [True] * n, n, cap=len(got) - 1) is None or not got
    assert top == sr.K_ENUM_CAP


def test_six_slots_agree_with_the_arithmetic_of_test_share_rule():
    """One rule, stated twice: tests/test_share_rule.py's subsets on its own random shares."""
    rng = np.random.default_rng(5)
    n, lim = 6, np.float32((1 - 0.37255) * (1 - 1e-6))
    rule = sr.Rule(0.1, 0.7, 1.0)
    rule.lim = lim
    seen = 0
    for _ in range(3000):
        q = rng.lognormal(np.log(30.0), 1.0, size=n) * (rng.random(n) > 0.05)
        rule.scale = 2.0 ** 20 / max(q.max() * 1.7, 3.0)
        qi = np.floor(q * rule.scale).astype(np.int64)
        thr = int(np.floor(np.float32(lim) * np.float32(qi.sum()))) - n - 2
        assert [int(x) for x in qi] == rule.shares(q)
        got = rule.asks([int(x) for x in qi], [False] * n, [True] * n, n)
        if thr <= 0:
            assert got is None
            continue
        bits = lambda m: [k for k in range(n) if m >> k & 1]
        heavy = {m for m in range(1, 1 << n) if qi[bits(m)].sum() >= thr}
        asked = {m for m in heavy if qi[bits(m)].sum() - qi[bits(m)].min() < thr}
        assert got == asked
        seen += 1
    assert seen > 2500


@pytest.mark.parametrize("n", [7, 8, 9, 10, 11, 12])
def test_run_by_run_every_heavy_agreeing_set_holds_a_mask_asked_for(n):
    """Random shares with slots that agree with anything and slots that agree with nothing: a set
    of agreeing slots (the wild ones among them) that holds the share `lim` of the real squared
    norms contains, in some run, a mask the window asks for -- or the window is not constrained."""
    rng = np.random.default_rng(100 + n)
    full = (1 << n) - 1
    constrained = with_wild = 0
    for trial in range(400):
        thr, gamma = sr.CONFIGS[trial % 3]
        q = rng.lognormal(np.log(30.0), 1.0, size=n) * (rng.random(n) > 0.05)
        rule = sr.Rule(thr, gamma, math.sqrt(q.max() * 1.3))
        kind = rng.random(n)
        wild = [bool(x < 0.12) for x in kind]
        usable = [bool(x >= 0.2) for x in kind]        # (between the two: a name, far from everything)
        qi = rule.shares(q)
        masks = rule.asks(qi, wild, usable, n)
        if masks is None:
            continue
        constrained += 1
        with_wild += any(wild)
        ok = sum(1 << k for k in range(n) if wild[k] or usable[k])
        for _ in range(60):
            agree = int(rng.integers(1, full + 1)) & ok
            if sum(q[k] for k in range(n) if agree >> k & 1) < float(rule.lim) * q.sum():
                continue
            assert any(m & ~agree == 0 for m in masks), (trial, agree)
    assert constrained > 150 and with_wild > 40
