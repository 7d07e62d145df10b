"""The cases of tests/refrains.py, checked without a GPU: the builder's invariants (the planned
forms and occurrences are in the script, the restated maps have the layout a case names, the
tie is bit-equal) and what the oracle returns for them (a record with a distance above 0.01
wherever a near window is planted, none on a window with two slots changed).  So the cases are
known good before test_gpu_refrains.py takes them to the device, and the branches that file
names are reached by the planted windows according to the restated maps."""

import numpy as np
import pytest

from tests import refrains as R


def script_holds(case):
    """Every form of every refrain occurs as often as planned."""
    n = case["n"]
    win = np.lib.stride_tricks.sliding_window_view(case["script"], n)
    for ref in case["refrains"]:
        for subst, occ in ref["forms"]:
            line = np.asarray(R._with(ref["base"], subst), dtype=np.uint32)
            assert int((win == line[None, :]).all(axis=1).sum()) == occ, (ref, subst)


def oracle_side(case, near=True):
    """Records with dist > 0.01 on a near window, none on a two-slot one; returns the rows."""
    rows, st = R.oracle_rows(case, threads=4)
    for fan in case["planted"]:
        if fan["kind"] == "two":
            assert len(R.rows_at(rows, fan)) == 0, fan
    if near:
        hits = [R.rows_at(rows, fan) for fan in case["planted"] if fan["kind"] == "near"]
        assert hits and any(len(r) and float(r["dist"].max()) > 0.01 for r in hits)
    return rows


def reached(case, names):
    got = R.predicted(case, every=False)               # (by the planted windows alone)
    for name in names:
        assert got.get(name, 0) > 0, (name, got)
    return got


# ---- the restatement ---------------------------------------------------------------------------

def test_restated_keys_scalar_and_vector_agree():
    rng = np.random.default_rng(5)
    for n in (6, 8, 10, 12):
        ids = rng.integers(0, 1 << 24, size=40)
        keys = R.all_window_keys(ids, n)
        for w in range(len(ids) - n + 1):
            assert [int(h) for h in keys[w]] == R.window_keys(ids[w:w + n])
    # two windows that differ in slot k have the same key k and no other
    a = [int(t) for t in rng.integers(0, 3000, size=8)]
    b = list(a)
    b[3] = a[3] + 1
    ka, kb = R.window_keys(a), R.window_keys(b)
    assert [x == y for x, y in zip(ka, kb)] == [k == 3 for k in range(8)]
    assert R.rotl(0x80000001, 0) == 0x80000001 and R.rotl(0x80000001, 1) == 3 and R.rot_of(5) == 3
    assert R.premix(0x1000001) == 0x9E3779 and R.wmap_slot(0xFFFFFFFF, 8) == (0x100000000 - 0x9E3779B1) >> 24


def test_restated_maps_take_the_entries_in_the_builders_order():
    """wmap by the n-grams in lexicographic order of their ids, emap in the memcmp order of their
    bytes (little-endian: the first id's low byte first); an entry's bucket follows from it."""
    n = 6
    script = np.array([0x100, 1, 2, 3, 4, 5, 9, 0x0FF, 1, 2, 3, 4, 5, 9, 0x001, 1, 2, 3, 4, 5], dtype=np.uint32)
    wmap, emap = R.layout_of(script, n)
    first = lambda m, w: m.entry[(w, 0)] // n
    assert sorted((0, 7, 14), key=lambda w: first(wmap, w)) == [14, 7, 0]       # 0x001 < 0x0FF < 0x100
    assert sorted((0, 7, 14), key=lambda w: first(emap, w)) == [0, 14, 7]       # low bytes 0x00 < 0x01 < 0xFF
    # the three n-grams differ in slot 0 only: one key, one home bucket, the entries in that order
    keys = {R.window_keys(script[w:w + n])[0] for w in (0, 7, 14)}
    assert len(keys) == 1 and {m.depth(w, 0, min(keys)) for m in (wmap, emap) for w in (0, 7, 14)} == {0}
    assert len(wmap.bucket) == len(emap.bucket) == n * len(R.distinct_grams(script, n)[0]) == n * 14   # (one n-gram twice)


def test_bucket_fill_does_not_depend_on_the_order():
    rng = np.random.default_rng(6)
    keys = [int(h) for h in rng.integers(0, 1 << 32, size=3000)]
    keys += keys[:40] * 3                          # crowded buckets, chains of full ones
    a = R.OneSlotMap(keys, 10)
    for seed in range(3):
        b = R.OneSlotMap([keys[i] for i in np.random.default_rng(seed).permutation(len(keys))], 10)
        assert (a.fill == b.fill).all()
    assert int(a.fill.sum()) == len(keys) and int(a.fill.max()) == 4 and int((a.fill == 4).sum()) > 40
    assert R.map_sizes(1000, 8) == (13, 14) and R.map_sizes(1, 6) == (8, 8) and R.map_sizes(1024, 8) == (13, 14)


# ---- the cases -----------------------------------------------------------------------------------

@pytest.mark.parametrize("v", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [8, 10])
def test_forms_in_one_slot(n, v):
    case = R.forms_case(n, v)
    script_holds(case)
    assert [ref["forms"][0][0].keys() for ref in case["refrains"]] == [{k} for k in R.slots_of(n)]
    for e in R.plan(case):
        if e["fan"]["kind"] in ("near", "far"):
            assert len(e["one_slot"]) == v and not e["is_gram"]
            assert all(g["dist"] > R.THR for g in e["one_slot"]) == (e["fan"]["kind"] == "far")
        elif e["fan"]["kind"] == "verbatim":
            assert e["is_gram"] and len(e["one_slot"]) == v - 1
        else:
            assert not e["one_slot"] and not e["is_gram"]
    reached(case, R.FORMS[v])
    oracle_side(case)


def test_slots_of_covers_the_group_borders():
    assert R.slots_of(8) == [0, 2, 3, 4, 5, 6, 7] and R.slots_of(10) == [0, 3, 4, 5, 6, 7, 9]
    assert R.slots_of(6) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("nearest_n", [10, 2])
@pytest.mark.parametrize("order", sorted(R.ORDERS))
@pytest.mark.parametrize("n", [8, 10])
def test_forms_at_different_slots(n, order, nearest_n):
    case = R.slots_case(n, order, nearest_n=nearest_n)
    script_holds(case)
    counts = []
    for e in R.plan(case):
        if e["fan"]["kind"] != "near":
            continue
        assert not e["is_gram"] and e["listed"] == e["one_slot"]
        slots = [g["slot"] for g in e["listed"]]
        assert slots == sorted(set(slots))                       # as many keys as n-grams
        rank = list(np.argsort(np.argsort([g["dist"] for g in e["listed"]])))
        assert rank == [r for r in R.ORDERS[order] if r < len(slots)]
        counts.append(len(slots))
    assert counts == [4, 4, 4, 3, 2]
    got = reached(case, ("enum_listed_2", "enum_listed_3", "enum_listed_4"))
    ranks = [[r for r in R.ORDERS[order] if r < count] for count in counts]
    assert got.get("enum_reordered", 0) == sum(r != sorted(r) for r in ranks) >= (0 if order == "ascending" else 4)
    assert got.get("enum_cut", 0) == sum(c > nearest_n for c in counts)      # (each n-gram once, in one table: UniqueFilter)
    rows = oracle_side(case)
    if nearest_n == 2:
        # fewer places than n-grams: the two nearest are kept, wherever they arrive
        for e in R.plan(case):
            if e["fan"]["kind"] == "near" and len(e["listed"]) > 2:
                kept = sorted(e["listed"], key=lambda g: g["dist"])[:2]
                got_rows = R.rows_at(rows, e["fan"])
                start = set((got_rows["orig_ix"] - (got_rows["fan_ix"] - e["fan"]["fan_ix"])).tolist())
                assert start <= {g["window"] for g in kept} and len(got_rows) == n


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("nearest_n", [1, 3, 10])
@pytest.mark.parametrize("n", [8, 10])
def test_occurrences_and_nearest_n(n, nearest_n, unique):
    case = R.occurrences_case(n, nearest_n, unique)
    script_holds(case)
    near = [e for e in R.plan(case) if e["fan"]["kind"] == "near"]
    assert [sorted(g["occ"] for g in e["listed"]) for e in near] == [sorted((occ, 2)) for occ in R.OCCURRENCES]
    wanted = [R.wanted_entries(e, unique, nearest_n) for e in near]
    assert any(w > nearest_n for w in wanted)
    first = [min(e["listed"], key=lambda g: g["dist"]) for e in near]
    assert [g["occ"] for g in first] == [1, 3, 2, 12]
    entries = [(1 if unique else len(g["tables"])) * g["occ"] for g in first]
    if nearest_n > 1 and unique:
        # the list is cut inside the nearer n-gram's entries, a second n-gram gets the places
        # that are left, and at N = 3 one list ends between the two n-grams
        assert any(x > nearest_n for x in entries)
        assert any(x < nearest_n < w for x, w in zip(entries, wanted))
        assert (nearest_n != 3) or any(x == nearest_n < w for x, w in zip(entries, wanted))
    if nearest_n == 10 and not unique:
        # ... and inside one table's occurrences: the list ends in the middle of a table's run
        assert any(x > nearest_n and nearest_n % g["occ"] for g, x in zip(first, entries))
    reached(case, ("enum_listed_2", "enum_cut"))
    oracle_side(case)


def test_tie():
    case = R.tie_case()
    script_holds(case)
    emb = case["emb"]
    y, x1, x2 = R.TIE_ROWS
    assert np.allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-6)
    cos = R.tie_table()[2]
    assert abs(cos[y, x1] - 0.5) < 1e-7 and cos[y, x1] == cos[y, x2] == cos.max()
    rows = oracle_side(case)
    for ref, k in zip(case["refrains"], R.slots_of(8)):
        f = R._with(ref["base"], {k: y})
        d1 = R.canonical_distance(emb, R._with(ref["base"], {k: x1}), f)
        d2 = R.canonical_distance(emb, R._with(ref["base"], {k: x2}), f)
        assert d1 == d2 and 0.01 < d1 < R.THR               # bit-equal, within the threshold
        fan = [p for p in case["planted"] if p["ids"] == f][0]
        assert set(R.rows_at(rows, fan)["dist"].tolist()) == {d1}
    for e in R.plan(case):
        if e["fan"]["kind"] == "near":
            assert len(e["listed"]) == 2
    reached(case, ("enum_giveup_tie",))


@pytest.mark.parametrize("length", [1, 2, 3])
@pytest.mark.parametrize("n", [8, 10])
def test_chains(n, length):
    case = R.chain_case(n, length)
    script_holds(case)
    wmap, emap = R.layout_of(case["script"], n)
    h = case["chain_key"]
    b = emap.home(h)
    assert emap.log2 == wmap.log2 + 1 and wmap.home(h) == b >> 1
    assert [int(emap.fill[(b + m) & emap.mask]) == 4 for m in range(length + 1)] == [True] * length + [False]
    assert wmap.fill[wmap.home(h)] == 4
    # the chain's buckets hold the stuffers' keys and the line's, nothing else at home there
    homes = {}
    for ref in case["refrains"]:
        for subst, _ in ref["forms"]:
            (k, _), = subst.items()
            key = R.window_keys(R._with(ref["base"], subst))[k]
            homes[emap.home(key)] = homes.get(emap.home(key), 0) + 1
    assert homes == {**{(b + m) & emap.mask: 4 for m in range(length)}, b: 5}
    # ... and the line's own entry went in behind theirs (its first id's low byte is 0xFF, theirs
    # are not: emap takes the n-grams in in the memcmp order of their ids): `length` buckets on
    at, k = case["chain_window"], case["chain_slot"]
    assert list(case["script"][at:at + n]) == R._with(case["refrains"][0]["base"], case["refrains"][0]["forms"][0][0])
    assert emap.depth(at, k, h) == length == case["chain_depth"]
    assert all(case["script"][at] & 0xFF == 0xFF > (ref["base"][0] & 0xFF) for ref in case["refrains"][1:])
    reached(case, (R.CHAINS[length], "wmap_pending_full_bucket"))
    rows = oracle_side(case)
    # the oracle's record on the near window is the line's: what the kernel must find at that follow
    near = [p for p in case["planted"] if p["kind"] == "near"][0]
    got = R.rows_at(rows, near)
    assert len(got) == n and (got["orig_ix"] - (got["fan_ix"] - near["fan_ix"]) == at).all()


@pytest.mark.parametrize("n", [8, 10])
def test_own_record(n):
    case = R.own_record_case(n)
    script_holds(case)
    for e in R.plan(case):
        assert e["is_gram"] and len(e["listed"]) == 1
    assert R.predicted(case, every=False) == {"record_with_neighbours": len(case["planted"])}
    rows = oracle_side(case, near=False)
    assert all(len(R.rows_at(rows, fan)) == n for fan in case["planted"])


@pytest.mark.parametrize("respellings", [2, 4, 5])
@pytest.mark.parametrize("n", [6, 8])
def test_component_ids(n, respellings):
    case = R.components_case(n, respellings)
    script_holds(case)
    cluster = case["key_ids"]
    for ref in case["refrains"]:
        lines = [R._with(ref["base"], s) for s, _ in ref["forms"]] + [R._with(ref["base"], ref["fans"][0][0])]
        ids = np.asarray(lines)
        assert (cluster[ids] == cluster[ids[0]][None, :]).all()         # the component ids are equal in all slots
        assert sorted((ids != ids[0][None, :]).sum(axis=1).tolist()) == [0] + [2] * respellings
    for e in R.plan(case):
        if e["fan"]["kind"] == "near":
            assert len(e["listed"]) == respellings and all(g["slot"] == -1 for g in e["listed"])
    assert set(R.COMPONENTS) == {2, 4, 5}
    oracle_side(case)


def test_share_rule_case():
    case = R.share_room_case()
    n = case["n"]
    win = np.lib.stride_tricks.sliding_window_view(case["script"], n)
    assert int((win == np.asarray(case["line"], dtype=np.uint32)[None, :]).all(axis=1).sum()) == 600
    fwin = np.lib.stride_tricks.sliding_window_view(case["tok"][:420], n)
    quoting = ((fwin == np.asarray(case["line"], dtype=np.uint32)[None, :]).sum(axis=1) >= n - 1)
    assert int(quoting.sum()) >= 50                  # copy after copy, some with a word swapped
    rows, st = R.oracle_rows(case, threads=4)
    assert int((rows["dist"] > 0.01).sum()) > 0 and len(rows) > 400
