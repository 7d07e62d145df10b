"""The share rule's kernels (k_share_scan<6 .. 12>, k_share_gate and the pairs' test in k_lsh_scan)
on window pairs built at the rule's bounds (tests/share_restated.py; test_share_bounds_host.py
proves on the CPU where they lie): records as the C oracle's, bit for bit, under three
(distance_threshold, FS_SHARE_GAMMA), with FS_LSH_SHARE 0, 3 and 43, and -- from an index that
counts -- the proof that the planted windows went through the rule and not around it.  Then the
stress generator's cases of nine, eleven and twelve slots (tools/stress_share.py), held against
the oracle here, not only against the key scan.

Six hash bits instead of fourteen: a pair at cosine 0.9 then shares one of fifteen buckets nearly
always, and the oracle alone reports nine in ten of the planted pairs within the threshold -- a
condition on the inputs, asserted from the oracle's rows."""

import importlib.util
import os

import numpy as np
import pytest

from fandom_search_amd import abi, synth
from fandom_search_amd.vocab import pack_strings
from tests import share_restated as sr
from tests import util

pytestmark = pytest.mark.gpu

H, B = 15, 6
_CASE = {}


def bounds_case(n, conf):
    """Inputs of one (n, configuration), and what only depends on them: the oracle's rows per
    unique_filter come later."""
    if _CASE.get("key") != (n, conf):
        b = sr.Bounds(n, *sr.CONFIGS[conf])
        strings, tok_str, swords = b.strings()
        chars, coff = pack_strings(strings)
        ex = sr.Exact(b)
        _CASE.clear()
        _CASE.update(key=(n, conf), b=b, tok_str=tok_str, swords=swords, chars=chars, coff=coff,
                     normals=synth.lsh_normals(n, H, B, dim=sr.D), within=[p for p in b.pairs if ex.is_record(p)],
                     free={False: b.unconstrained_windows(False), True: b.unconstrained_windows(True)})
    return _CASE


def keys_of(rows):
    return set(zip(rows["work"].tolist(), rows["fan_ix"].tolist(), rows["orig_ix"].tolist()))


@pytest.mark.parametrize("unique", [0, 1])
@pytest.mark.parametrize("conf", range(len(sr.CONFIGS)), ids=lambda c: "thr%g-gamma%g" % sr.CONFIGS[c])
@pytest.mark.parametrize("n", sr.SIZES)
def test_pairs_at_the_bounds_equal_oracle(n, conf, unique, monkeypatch):
    from oracle import c_oracle
    from fandom_search_amd.engine import ScriptIndex
    thr, gamma = sr.CONFIGS[conf]
    x = bounds_case(n, conf)
    b, tok_str, swords, chars, coff, normals = x["b"], x["tok_str"], x["swords"], x["chars"], x["coff"], x["normals"]
    cfg = abi.make_config(window_size=n, number_of_hashes=H, hash_dimensions=B, distance_threshold=thr,
                          emb_dim=sr.D, unique_filter=unique)
    sch, so = pack_strings(swords)
    oi = c_oracle.OracleIndex(cfg, b.script, sch, so, b.emb, normals, threads=8)
    want, ost = oi.search(b.tok, b.off, chars, coff, tok_str=tok_str)
    oi.close()
    # the inputs: of the planted pairs within the threshold the oracle reports nine in ten
    # (a pair: the n words of its window against the n of its script window; the windows one word
    # to either side share n - 1 of them and may be records of their own, with n - 1 of these rows)
    words = lambda p: {(p.work, p.f_at + k, p.s_at + k) for k in range(n)}
    seen = keys_of(want)
    reported = [p for p in x["within"] if words(p) <= seen]
    assert len(x["within"]) > len(b.pairs) // 5 and len(reported) >= 0.9 * len(x["within"])

    monkeypatch.setenv("FS_SHARE_GAMMA", repr(gamma))
    monkeypatch.delenv("FS_LSH_SHARE", raising=False)
    monkeypatch.delenv("FS_SHARE_COUNT", raising=False)

    def search(share=None, count=False):
        if share is not None:
            monkeypatch.setenv("FS_LSH_SHARE", share)
        if count:
            monkeypatch.setenv("FS_SHARE_COUNT", "1")
        ix = ScriptIndex(b.script, swords, b.emb, normals, cfg=cfg)
        monkeypatch.delenv("FS_LSH_SHARE", raising=False)
        monkeypatch.delenv("FS_SHARE_COUNT", raising=False)
        c = ix.corpus(b.tok, b.off, chars, coff, tok_str=tok_str)
        got, st = ix.search(c)
        return ix, c, got, st

    ix, c, got, st = search()
    info = ix.share_info()
    assert ix.kernel_name(c) == "k_share_scan<%d>" % n and info["flags"] & 32 and not info["flags"] & 8
    assert info["gamma"] == gamma
    # the components are the builder's: the twins at gamma - 1.2e-4 (and - 2e-4, - 1e-3) two, those
    # at gamma + 1e-3 one, every parallel group one, the zero rows and the fan text's filler alone
    sizes, used = ix.component_sizes()
    assert used and sorted(int(s) for s in sizes) == b.component_sizes()
    util.assert_rows_equal(got, want)
    assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
    have = keys_of(got)
    for p in reported:
        assert words(p) <= have, p
    ix.close()
    # the key scan; the gate and the pairs' test inside it; names that agree with anything
    for share, kernel in (("0", "k_lsh_scan"), ("3", "k_lsh_scan"), ("43", "k_share_scan<%d>" % n)):
        ix2, c2, got2, st2 = search(share)
        assert ix2.kernel_name(c2) == kernel, share
        assert got2.tobytes() == got.tobytes() and st2.matches == st.matches, share
        ix2.close()
    # proof of reach: what passed what
    for share, all_wild in ((None, False), ("43", True)):
        ixc, cc, gotc, stc = search(share, count=True)
        ixc.share_counts()                             # (the counters add up until they are read: that search may have run twice for room)
        gotc, stc = ixc.search(cc, cap=len(got) + 1024)
        cnt = ixc.share_counts()
        assert gotc.tobytes() == got.tobytes()
        assert bool(ixc.share_info()["flags"] & 8) == all_wild
        assert cnt["windows"] == len(b.tok) - n + 1
        assert cnt["windows_flagged_as_they_are"] == x["free"][all_wild], (share, cnt)
        assert x["free"][all_wild] >= (1 + len(b.runs) if all_wild or b.script_names else 0)
        assert cnt["pairs_tested"] > cnt["distances"] > 0
        assert 0 < cnt["windows_with_a_key_in_the_filter"] < cnt["windows"]
        ixc.close()


def _stress():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "stress_share.py")
    spec = importlib.util.spec_from_file_location("stress_share", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [9, 11, 12])
def test_stress_cases_of_three_runs_equal_oracle(n, monkeypatch):
    """The generator's planted spans (the lightest slots replaced), names on both sides, norms
    around 1: windows of nine slots in two runs, of eleven and twelve in three, 16-bit masks."""
    from oracle import c_oracle
    from fandom_search_amd.engine import ScriptIndex
    x = _stress().case_inputs(case=n, rows=1500, sigma=0.3, n=n, thr=0.1, gamma=0.7, oov=0.08, scale=0.15,
                              n_script=400, n_works=3, per=200, names=True, unique=bool(n % 2),
                              rng=np.random.default_rng(n))
    sch, so = pack_strings(x["swords"])
    oi = c_oracle.OracleIndex(x["cfg"], x["script"], sch, so, x["emb"], x["normals"], threads=8)
    want, ost = oi.search(x["tok_vec"], x["off"], x["chars"], x["coff"], tok_str=x["tok_str"])
    oi.close()
    monkeypatch.setenv("FS_SHARE_GAMMA", "0.7")
    rows = {}
    for share in ("35", "0"):
        monkeypatch.setenv("FS_LSH_SHARE", share)
        ix = ScriptIndex(x["script"], x["swords"], x["emb"], x["normals"], cfg=x["cfg"])
        c = ix.corpus(x["tok_vec"], x["off"], x["chars"], x["coff"], tok_str=x["tok_str"])
        rows[share], st = ix.search(c)
        assert ix.kernel_name(c) == ("k_share_scan<%d>" % n if share == "35" else "k_lsh_scan")
        assert st.matches == ost.matches and st.windows_processed == ost.windows_processed
        ix.close()
    util.assert_rows_equal(rows["35"], want)
    assert rows["0"].tobytes() == rows["35"].tobytes() and len(want) > 0
