"""The hostile inputs of tests/keys_restated.py bite, proved without a GPU.

For every case of test_gpu_hostile_keys.py:
  * the float64 restatement's script keys are the C oracle's (fo_script_keys, as
    test_oracle_known_answers.py reads them);
  * the planted windows are what the case says (keys_restated.assert_planted: the condition
    every GPU case rests on);
  * the Python oracle (oracle/search_restated.py, canonical arithmetic) gives the C oracle's
    records, with every polarity-1 window's record present and every polarity-2 window's absent;
  * the same oracle with the fan windows' keys replaced by the float32 signs gives records that
    differ in exactly the words of the planted windows: each one's record is present or absent
    the other way round;
  * with the keys as the kernels decide them at FS_LSH_F32_SLACK=0 (a float32 sum that is not 0 is
    trusted) the records differ in exactly the FLIPPED windows -- what the device must show
    under that switch -- and at the default slack they are the oracle's.
"""

import numpy as np
import pytest

from oracle import nearpy_restated as nr
from oracle import search_restated as sr
from tests import keys_restated as K
from tests import util

ALL = sorted(K.CASES) + sorted(K.OOV_CASES)


def c_oracle_index(case):
    return util.oracle_index(case["cfg"], case["script"], None, case["emb"], case["normals"], threads=4,
                             swords=case["swords"])


def c_rows(case):
    oi = c_oracle_index(case)
    rows, _ = oi.search(case["tok"], case["off"], case["chars"], case["coff"], tok_str=case["tok_str"])
    oi.close()
    return rows


class PresetKeys(object):
    """A hash of the engine that answers the windows of a work, in order, with given keys."""

    def __init__(self, name, bits):
        self.hash_name, self.bits, self.keys = name, bits, iter(())

    def hash_vector(self, win):
        return [format(int(next(self.keys)), "0%db" % self.bits)]


def python_rows(case, fan_keys=None):
    """Records of the Python oracle as an abi.ROW_DTYPE array; fan_keys[w][h]: the keys of the
    fan windows (by position in the token stream) in the place of the canonical ones."""
    from fandom_search_amd import abi
    strings, d = case["strings"], case["emb"].shape[1]

    def tok(t, sid):
        if int(t) & abi.FS_OOV_FLAG:
            vec = np.zeros(d, dtype=np.float32)
            vec[list(K.oov_hot(t, d))] = 1.0
        else:
            vec = case["emb"][int(t)]
        return sr.Tok(strings[sid], sid, strings[sid], sid, vec)

    script = [tok(t, strings.index(w)) for t, w in zip(case["script"], case["swords"])]
    rows = [[t.orth_, t.orth, 0, "c"] for t in script]
    cfg = case["cfg"]
    idx = sr.AnnIndexSearch(rows, script, case["n"], case["h"], case["b"], cfg.distance_threshold,
                            case["normals"], arith=nr.CanonicalArith(), unique_filter=bool(cfg.unique_filter),
                            nearest=cfg.nearest_n)
    if fan_keys is not None:
        idx.engine.lshashes = [PresetKeys(h.hash_name, case["b"]) for h in idx.engine.lshashes]
    out = []
    off = [int(x) for x in case["off"]]
    for w in range(len(off) - 1):
        fan = [tok(t, s) for t, s in zip(case["tok"][off[w]:off[w + 1]], case["tok_str"][off[w]:off[w + 1]])]
        if fan_keys is not None:
            for h, preset in enumerate(idx.engine.lshashes):
                preset.keys = iter(fan_keys[off[w]:off[w + 1] - case["n"] + 1, h])
        out += [(w, r[1], r[4], r[10], r[9], r[11]) for r in idx.search(w, fan)]
    return np.array(out, dtype=abi.ROW_DTYPE)


@pytest.fixture(scope="module")
def facts():
    """Per case, computed once: the restated keys and the C oracle's records."""
    store = {}

    def get(name):
        if name not in store:
            case = K.case(name)
            store[name] = dict(case=case, keys=K.case_keys(case), want=c_rows(case))
        return store[name]
    return get


@pytest.mark.parametrize("name", ALL)
def test_script_keys_equal_the_c_oracle(name, facts):
    f = facts(name)
    oi = c_oracle_index(f["case"])
    got = np.stack([oi.script_keys(w) for w in range(len(f["case"]["script"]) - f["case"]["n"] + 1)])
    oi.close()
    assert (got == f["keys"]["script"]).all()


@pytest.mark.parametrize("name", ALL)
def test_planted_windows_are_hostile(name, facts):
    f = facts(name)
    count = K.assert_planted(f["case"], f["keys"])
    print(name, "flipped %d zero %d nonfinite %d" % (count[K.FLIPPED], count[K.ZERO], count[K.NONFINITE]))


@pytest.mark.parametrize("name", ALL)
def test_records_turn_with_the_hostile_bit(name, facts):
    f = facts(name)
    case, keys, want = f["case"], f["keys"], f["want"]
    n = case["n"]
    # float64 keys: the expected records
    util.assert_rows_equal(python_rows(case), want)
    have = {(int(r["work"]), int(r["fan_ix"])): int(r["orig_ix"]) for r in want}
    for p in case["planted"]:
        for k in range(n):
            at = have.get((p["work"], p["fan_ix"] + k))
            assert at == (p["orig_ix"] + k if p["polarity"] == 1 else None), (p, k, at)
    # the restated float64 keys in the canonical ones' place: the same records
    util.assert_rows_equal(python_rows(case, keys["k64"]), want)
    # float32 keys: every planted window the other way round, nothing else
    if not case["overflow"]:
        turned = python_rows(case, keys["k32"])
        assert K.differing_words(turned, want) == K.planted_words(case)
        have = {(int(r["work"]), int(r["fan_ix"])): int(r["orig_ix"]) for r in turned}
        for p in case["planted"]:
            for k in range(n):
                at = have.get((p["work"], p["fan_ix"] + k))
                assert at == (p["orig_ix"] + k if p["polarity"] == 2 else None), (p, k, at)
    # as decided at slack 0: the FLIPPED windows turn, the ZERO (and NONFINITE) ones fall back
    k0 = K.case_keys(case, slack=0.0)["kdec"]
    assert K.differing_words(python_rows(case, k0), want) == K.planted_words(case, (K.FLIPPED,))
    # as decided at the default slack: the oracle's records
    util.assert_rows_equal(python_rows(case, keys["kdec"]), want)
