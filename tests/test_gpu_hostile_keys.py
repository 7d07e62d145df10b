"""GPU parity of the float32 LSH key signs on windows whose projection cancels
(tests/keys_restated.py; test_keys_restated_host.py proves on the CPU that the inputs bite).

The decision "trust the float32 sign iff |sum| > bound" is written out in four places:
lsh_window (k_lsh_verify, k_lsh_gramtab, the crowded windows of k_lsh_batch), k_lsh_batch,
k_lsh_pkeys and k_lsh_scan.  On random projections a float32 sum never lands near zero, so a
bound far too tight, a column mask that drops the last lane's columns or a lane that skips the
vote would change no record.  Here every case plants at least 8 windows whose float32 sum on
one column has the wrong sign (FLIPPED) and 8 whose float32 sum is 0 (ZERO), each next to a
script line that the window reaches through that column's table alone: a wrong bit makes a
record appear or disappear.  The condition is asserted from the restatement before the search.

  each of the four sites        test_site_equals_oracle: the switches of keys_restated.SITES, the
                                launch list (and FS_LSH_COUNT's counters for k_lsh_enum) saying
                                that the intended kernel took the planted windows
  the hostile column            0, 3, 4, C - 1 at C = 1, 150 (the last lane holds 2 live columns
                                and 2 padded ones), 255, 256; C = 272 is the float64-only
                                control of lsh_window, k_lsh_batch and k_lsh_pkeys
  the cancelling slots          0 and 1, the last two, the first against the last two, n = 6, 8, 10
  OOV windows                   the sum inside row32: three hot positions, two coinciding, two
                                OOV tokens in a window; with and without FS_LSH_DIAG=64
  scale                         projections in the float32 subnormal range (the bound needs an
                                absolute term there), rows that overflow float32
  proof of reach                every search once more with FS_LSH_F32_SLACK=0 (a float32 sum that
                                is not 0 is trusted): the records differ from the oracle's in
                                exactly the FLIPPED windows.  A case that stays equal there did
                                not reach the float32 path.

Every search is bit-compared with the plain-C oracle.
"""

import numpy as np
import pytest

from fandom_search_amd import abi
from tests import keys_restated as K
from tests import util

pytestmark = pytest.mark.gpu

ALL = sorted(K.CASES)
GEN = abi.FS_MODE_GENERAL


@pytest.fixture(scope="module")
def oracle():
    """Per case, computed once and left alone: the inputs, the C oracle's records and stats."""
    from oracle import c_oracle
    from fandom_search_amd.vocab import pack_strings
    store = {}

    def get(name):
        if name not in store:
            case = K.case(name)
            K.assert_planted(case)
            sch, so = pack_strings(case["swords"])
            oi = c_oracle.OracleIndex(case["cfg"], case["script"], sch, so, case["emb"], case["normals"], threads=8)
            want, ost = oi.search(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])
            oi.close()
            store[name] = (case, want, ost)
        return store[name]
    return get


def launches(ix, corpus, n_rows):
    """Kernel names of one profiled search of `corpus` (fs_search_profile)."""
    import torch
    cap = n_rows + 1024
    buf = torch.zeros(32 * cap + 64, dtype=torch.uint8, device="cuda")
    names = [k for k, _ in ix.profile(corpus, buf.data_ptr() + 32, cap)]
    torch.cuda.synchronize()
    return names


def search(case, env, monkeypatch):
    """One index built under `env` (the switches are read then) and one search of the case's works."""
    from fandom_search_amd.engine import ScriptIndex
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ix = ScriptIndex(case["script"], case["swords"], case["emb"], case["normals"], cfg=case["cfg"])
    for k in env:
        monkeypatch.delenv(k)
    c = ix.corpus(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])
    got, st = ix.search(c)
    return ix, c, got.copy(), st


def check(name, env, monkeypatch, oracle, reach=True):
    """Records as the oracle's under `env`; under `env` and FS_LSH_F32_SLACK=0 they differ from the
    oracle's in the words of the FLIPPED windows and nowhere else (`reach`; False: in none, the
    float32 path is not taken there).  Returns the first index, its corpus and stats."""
    case, want, ost = oracle(name)
    ix, c, got, st = search(case, env, monkeypatch)
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
    assert ix.info["path"] == GEN and st.path == GEN
    # the planted windows stay pending: all of them behind the prefilter; behind k_lsh_scan (no
    # prefilter: the switch, or OOV tokens), which keeps the windows that have a script window within
    # the threshold in a shared bucket, those of polarity 1
    scanned = "FS_LSH_PREFILTER" in env or name in K.OOV_CASES
    assert st.lsh_pending >= sum(1 for p in case["planted"] if p["polarity"] == 1 or not scanned)
    ix0, _, got0, _ = search(case, dict(env, FS_LSH_F32_SLACK="0"), monkeypatch)
    ix0.close()
    turned = K.planted_words(case, (K.FLIPPED,)) if reach else set()
    assert K.differing_words(got0, want) == turned
    return case, ix, c, st, got


# ---- the four sites -----------------------------------------------------------------

@pytest.mark.parametrize("site", sorted(K.SITES))
def test_site_equals_oracle(site, monkeypatch, oracle):
    env, present, absent = K.SITES[site]
    case, ix, c, st, got = check("base", env, monkeypatch, oracle)
    names = launches(ix, c, len(got))
    ix.close()
    for k in present:
        assert any(x.startswith(k) for x in names), (k, names)
    for k in absent:
        assert not any(x.startswith(k) for x in names), (k, names)
    if site == "pkeys":
        # k_lsh_enum works from k_lsh_pkeys' keys and leaves no window to k_lsh_batch; it lists
        # the windows that share a key with their script n-gram one slot away: those of polarity
        # 1, and no other window of these works has such an n-gram
        ixc, _, gotc, stc = search(case, dict(env, FS_LSH_COUNT="1"), monkeypatch)
        counts = ixc.lsh_counts()
        ixc.close()
        print(counts, stc.lsh_pending)
        assert gotc.tobytes() == got.tobytes()
        assert counts["enum_listed_1"] == sum(1 for p in case["planted"] if p["polarity"] == 1)
        assert sum(counts["enum_listed_%d" % k] for k in (2, 3, 4)) == 0
        assert counts["enum_giveup_fifth"] == counts["enum_giveup_chain"] == counts["enum_giveup_tie"] == 0


# ---- columns, slots, scale ------------------------------------------------------------

@pytest.mark.parametrize("site", K.MAIN_SITES)
@pytest.mark.parametrize("name", [x for x in ALL if x != "base"])
def test_case_equals_oracle(name, site, monkeypatch, oracle):
    env = K.SITES[site][0]
    case = K.case(name)
    # (C = 272: float64 only in lsh_window, k_lsh_batch and k_lsh_pkeys; k_lsh_scan takes the
    # columns 256 at a time -- tested by parity alone.  Rows beyond float32: nothing to trust)
    reach = case["h"] * case["b"] <= 256 and not case["overflow"]
    if name == "c272_last" and site == "scan":
        # k_lsh_scan by itself: at slack 0 it trusts column 271 (its second round of columns), while
        # the kernels behind it work in float64.  A FLIPPED window of polarity 1 is then not flagged
        # and its record is lost; one of polarity 2 is flagged, and the float64 keys behind find
        # nothing, as the oracle.
        case, want, _ = oracle(name)
        ix, _, got, _ = search(case, env, monkeypatch)
        ix.close()
        util.assert_rows_equal(got, want)
        ix0, _, got0, _ = search(case, dict(env, FS_LSH_F32_SLACK="0"), monkeypatch)
        ix0.close()
        lost = {(p["work"], p["fan_ix"] + k) for p in case["planted"]
                if p["kind"] == K.FLIPPED and p["polarity"] == 1 for k in range(case["n"])}
        assert K.differing_words(got0, want) == lost
        return
    _, ix, _, _, _ = check(name, env, monkeypatch, oracle, reach=reach)
    ix.close()


# ---- OOV windows ----------------------------------------------------------------------

@pytest.mark.parametrize("envname", sorted(K.OOV_ENVS))
@pytest.mark.parametrize("name", sorted(K.OOV_CASES))
def test_oov_case_equals_oracle(name, envname, monkeypatch, oracle):
    # (FS_LSH_DIAG=64 sends every window with an OOV token to float64: nothing turns at slack 0)
    _, ix, _, _, _ = check(name, K.OOV_ENVS[envname], monkeypatch, oracle, reach="diag64" not in envname)
    ix.close()
