"""GPU parity of the one-slot maps on scripts that repeat a line with a word changed
(tests/refrains.py).  Two script n-grams one slot apart share the key of that slot and so a bucket
of four of `wmap` (sift_stage2 of fs_lsh_sift.hip), of `emap` / `emapc` (k_lsh_enum) -- the one
place where those maps branch on their data, and one that a script of independent draws never
reaches.  Every case is compared with the plain-C oracle bit for bit, byte for byte with the same
index built under FS_LSH_PREFILTER=0, FS_LSH_EMAP=0 and FS_LSH_WMAP=0, with k_lsh_enum on the
launch list (FS_LSH_DEFER_MIN=0 and a string table: it runs however few windows are pending), and
names the counters (FS_LSH_COUNT=1, ScriptIndex.lsh_counts) of the branches it is there for: a
case that stops reaching its branch fails.  Where the maps are keyed by vector ids the counters
are held against what tests/refrains.predicted works out from the restated maps for every window of
the fan works: equal where a window needs a script n-gram one slot away to get there (refrains.EXACT:
a counter that counted twice, or under a second name as well, fails), at least that where a false
positive of the filters in front can get there too; and no counter may exceed the windows that can
reach it (candidates, pending windows).

Branch (counter)                                         cases
  sift_stage2, the n-gram's own record
    with further matches (record_with_neighbours)        own_record, forms V >= 2 at n = 10
  sift_stage2, wmap
    ended with 1 / 2 n-grams (wmap_ended_1, _2)          forms V = 1 / V = 2, the far window
    pending by a distance (wmap_pending_distance)        forms V = 1, 2, the near window; occurrences; tie
    pending by nh > 2 (wmap_pending_many)                forms V = 3; slots
    pending by a full bucket (wmap_pending_full_bucket)  forms V = 4, 5 (the spilt entry); chain
  k_lsh_enum, emap
    lists of 1 .. 4 n-grams (enum_listed_1 .. _4)        forms V = 1 .. 4; slots (2, 3, 4 keys)
    the sort exchanges two n-grams (enum_reordered)      slots: descending, interleaved_a, interleaved_b;
                                                         0 on ascending.  At N = 1, 2, 3 the list has
                                                         fewer places than n-grams: the sorted order
                                                         decides which are kept (records as the oracle's)
    the list cut at N (enum_cut)                         occurrences: inside an n-gram's entries, inside
                                                         one table's occurrences, the second n-gram
                                                         taking the places left; UniqueFilter on and off
    occurrences per table bit, first table only          occurrences (parity with the oracle)
    a chain followed once / twice (enum_chain_once,
      enum_chain_twice)                                  forms V = 4, 5; chain 1 / chain 2: the line's own
                                                         entry one / two buckets from home (the restated
                                                         map puts the entries in in emap's order and says
                                                         so), the record only there to be found
    give-up by a fifth n-gram (enum_giveup_fifth)        forms V = 5 (k_lsh_batch takes the windows);
                                                         components, 5 respellings
    give-up by the chain (enum_giveup_chain)             chain 3: the entry three buckets from home
    give-up by a tie (enum_giveup_tie)                   tie
  k_lsh_enum, emapc (component ids, no wmap)             components: 2, 4, 5 respellings at n = 6, 8
  k_share_scan, no room in the workgroup's lists
    (share_counts: windows_flagged_as_they_are)          share_room
"""

import numpy as np
import pytest

from fandom_search_amd import abi
from tests import refrains as R
from tests import util

pytestmark = pytest.mark.gpu

SWITCHED_OFF = ({"FS_LSH_PREFILTER": "0"}, {"FS_LSH_EMAP": "0"}, {"FS_LSH_WMAP": "0"})


def launches(ix, corpus, n_rows):
    """Kernel names of one profiled search of `corpus` (fs_search_profile)."""
    import torch
    cap = n_rows + 1024
    buf = torch.zeros(32 * cap + 64, dtype=torch.uint8, device="cuda")
    names = [k for k, _ in ix.profile(corpus, buf.data_ptr() + 32, cap)]
    torch.cuda.synchronize()
    return names


def check(case, monkeypatch, reached, absent=(), kernel="k_lsh_enum"):
    """Records as the oracle's and as the switched-off builds'; returns the counters of one
    search of an index that counts."""
    from fandom_search_amd.engine import ScriptIndex
    monkeypatch.setenv("FS_LSH_DEFER_MIN", "0")
    cfg = R.config_of(case)
    want, ost = R.oracle_rows(case)

    def build(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)             # switches are read when the index is built
        ix = ScriptIndex(case["script"], case["swords"], case["emb"], case["normals"], cfg=cfg)
        for k in env:
            monkeypatch.delenv(k)
        return ix, ix.corpus(case["tok"], case["off"], case["chars"], case["coff"])

    ix, c = build({})
    got, st = ix.search(c)
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.path == abi.FS_MODE_GENERAL
    names = launches(ix, c, len(got))
    assert any(k.startswith(kernel) for k in names), (kernel, names)
    assert not any(ix.lsh_counts().values())             # (counters are off unless FS_LSH_COUNT is set)
    ix.close()
    for env in SWITCHED_OFF:
        ix2, c2 = build(env)
        got2, st2 = ix2.search(c2)
        assert got2.tobytes() == got.tobytes() and st2.matches == st.matches, env
        ix2.close()
    ixc, cc = build({"FS_LSH_COUNT": "1"})
    gotc, stc = ixc.search(cc)
    assert gotc.tobytes() == got.tobytes() and stc.matches == st.matches
    counts = ixc.lsh_counts()
    assert not any(ixc.lsh_counts().values())            # (read and cleared)
    ixc.close()
    print(counts)
    if case["key_ids"] is None and case["planted"]:
        # what the restated maps say of every window of the fan works: exact where a window needs a
        # script n-gram one slot away to get there, a lower bound where a false positive of the
        # filters in front can get there too
        want_counts = R.predicted(case)
        for name in R.EXACT:
            assert counts[name] == want_counts.get(name, 0), (name, want_counts, counts)
        for name, least in want_counts.items():
            assert counts[name] >= least, (name, least, counts)
    # a window is in one of the second stage's counters at most, a pending window listed once at most
    sift = ("record_with_neighbours", "record_alone", "wmap_ended_0", "wmap_ended_1", "wmap_ended_2",
            "wmap_pending_distance", "wmap_pending_many", "wmap_pending_full_bucket")
    assert sum(counts[k] for k in sift) <= stc.candidates
    assert sum(counts[k] for k in sift[5:]) <= stc.lsh_pending
    listed = sum(counts["enum_listed_%d" % k] for k in (1, 2, 3, 4))
    gave_up = [counts[k] for k in ("enum_giveup_fifth", "enum_giveup_chain", "enum_giveup_tie")]
    assert listed + max(gave_up) <= stc.lsh_pending and sum(gave_up) + listed <= 3 * stc.lsh_pending
    assert counts["enum_reordered"] + counts["enum_listed_1"] <= listed and counts["enum_cut"] <= listed
    assert counts["enum_chain_once"] + counts["enum_chain_twice"] + counts["enum_giveup_chain"] <= stc.lsh_pending
    for name in reached:
        assert counts[name] > 0, (name, counts)
    for name in absent:
        assert counts[name] == 0, (name, counts)
    return counts


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("v", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n", [8, 10])
def test_forms_in_one_slot(n, v, unique, monkeypatch):
    """V forms of a line in one slot, each once, at slot 0, the middle, n - 1 and on both sides of
    the borders of fs_wild_group; the fan window with a near word there, and with a far one."""
    check(R.forms_case(n, v, unique), monkeypatch, R.FORMS[v])


@pytest.mark.parametrize("nearest_n,unique", [(10, 1), (10, 0), (1, 1), (2, 1), (3, 1)])
@pytest.mark.parametrize("order", sorted(R.ORDERS))
@pytest.mark.parametrize("n", [8, 10])
def test_forms_at_different_slots(n, order, nearest_n, unique, monkeypatch):
    """The fan window one slot from two, three and four script n-grams through as many keys, their
    distances arriving in the order the case names.  At N = 1, 2, 3 (every n-gram once, the
    UniqueFilter on) the list has fewer places than n-grams: the sorted order decides which of
    them are kept, and the records show it."""
    check(R.slots_case(n, order, unique, nearest_n=nearest_n), monkeypatch,
          ("enum_listed_2", "enum_listed_3", "enum_listed_4") + (() if order == "ascending" else ("enum_reordered",)) +
          (("enum_cut",) if nearest_n < 10 else ()))


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("nearest_n", [1, 3, 10])
@pytest.mark.parametrize("n", [8, 10])
def test_occurrences_and_nearest_n(n, nearest_n, unique, monkeypatch):
    """A form 1, 3, 10 and 12 times in the script next to a second form, N = 1, 3, 10."""
    check(R.occurrences_case(n, nearest_n, unique), monkeypatch, ("enum_listed_2", "enum_cut"))


@pytest.mark.parametrize("unique", [1, 0])
def test_tie(unique, monkeypatch):
    """Two listed n-grams at bit-equal distance: left to the bucket walk, where the first arrival
    wins by table order."""
    check(R.tie_case(unique), monkeypatch, ("enum_giveup_tie", "wmap_pending_distance"))


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("length", [1, 2, 3])
@pytest.mark.parametrize("n", [8, 10])
def test_chains(n, length, unique, monkeypatch):
    """The line's key at home in a bucket that starts a chain of one, two, three full buckets of
    emap (and in a full bucket of wmap)."""
    case = R.chain_case(n, length, unique)
    wmap, emap = R.layout_of(case["script"], n)
    assert emap.chain(case["chain_key"]) == length and wmap.chain(case["chain_key"]) >= 1
    # the line's own entry lies `length` buckets from home: found at that follow, or given up
    assert emap.depth(case["chain_window"], case["chain_slot"], case["chain_key"]) == length
    check(case, monkeypatch, (R.CHAINS[length], "wmap_pending_full_bucket"))


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("n", [8, 10])
def test_own_record(n, unique, monkeypatch):
    """The fan window is a script form verbatim, other forms within the threshold."""
    check(R.own_record_case(n, unique), monkeypatch, ("record_with_neighbours",))


@pytest.mark.parametrize("unique", [1, 0])
@pytest.mark.parametrize("respellings", [2, 4, 5])
@pytest.mark.parametrize("n", [6, 8])
def test_component_ids(n, respellings, unique, monkeypatch):
    """The clustered table: a line in 2, 4 and 5 respellings, the fan window yet another -- the
    same component ids in all n slots, so all n keys in the same buckets of emapc."""
    counts = check(R.components_case(n, respellings, unique), monkeypatch, R.COMPONENTS[respellings])
    # (keyed by component ids: no wmap)
    assert not any(v for k, v in counts.items() if k.startswith("wmap_"))


def test_share_rule_has_no_room(monkeypatch):
    """A line 600 times in the script and copy after copy in a fan work: more keys in the filter
    than a workgroup of k_share_scan has room for."""
    from fandom_search_amd.engine import ScriptIndex
    case = R.share_room_case()
    cfg = R.config_of(case)
    want, ost = R.oracle_rows(case)
    monkeypatch.setenv("FS_SHARE_COUNT", "1")
    ix = ScriptIndex(case["script"], case["swords"], case["emb"], case["normals"], cfg=cfg)
    monkeypatch.delenv("FS_SHARE_COUNT")
    c = ix.corpus(case["tok"], case["off"], case["chars"], case["coff"])
    assert ix.kernel_name(c) == "k_share_scan<6>"
    got, st = ix.search(c)
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches
    counts = ix.share_counts()
    print(counts)
    assert counts["windows_flagged_as_they_are"] > 0
    ix.close()
    monkeypatch.setenv("FS_LSH_SHARE", "0")              # the key scan over every window: the same bytes
    ix2 = ScriptIndex(case["script"], case["swords"], case["emb"], case["normals"], cfg=cfg)
    c2 = ix2.corpus(case["tok"], case["off"], case["chars"], case["coff"])
    got2, st2 = ix2.search(c2)
    assert ix2.kernel_name(c2) == "k_lsh_scan" and got2.tobytes() == got.tobytes() and st2.matches == st.matches
    ix2.close()
