"""`saturation` on the GPU: fs_saturation and fs_saturation_rows against the restated contract
(tests/saturation_restated.py), every field of every output and the first times themselves
compared for equality, with the product reading the table of times (FS_SATURATION_TABLE=1) and
hashing in the lane (0), its words in one share (FS_SATURATION_KSPLIT=1) and in three, a wave
taking all the chunks of 64 orders of its row (FS_SATURATION_OSPLIT=1) and half of them; active
works, units, orders and points around every size the kernels treat differently; an incidence
that no swap of unit and work or of order and unit leaves unchanged; `ao3.py saturation` byte
for byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, intervals, saturation, synth
from fandom_search_amd.cli import main
from tests import saturation_restated as sr
from tests.golden import make_saturation_golden as msg
from tests.test_gpu_companions import on_device
from tests.test_gpu_pairs import from_spans, interleaved

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
N_SCRIPT = 3000          # of the index behind fs_saturation_rows; every case uses it
WIDTH = 3                # script words of a unit in the synthetic cases, and their --min-words
SWITCHES = ("FS_SATURATION_TABLE", "FS_SATURATION_KSPLIT", "FS_SATURATION_OSPLIT")
# both sources of a time with one and three shares of a row's words; a wave taking every chunk
# of 64 orders of its row (OSPLIT 1) and every second one; and what the library chooses
PATHS = [{"FS_SATURATION_TABLE": t, "FS_SATURATION_KSPLIT": k, "FS_SATURATION_OSPLIT": o}
         for t, k, o in ("111", "132", "012", "031")] + [{}]
DTYPES = (np.dtype(np.uint32), abi.SATURATION_POINT_DTYPE, abi.SATURATION_PERM_DTYPE,
          abi.SATURATION_SUMMARY_DTYPE, np.dtype(np.uint32))


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, m, g, R, K, seed, level):
    recs = list(zip(*(c.tolist() for c in cols)))
    works, pts, perms, summary, first = sr.saturation(
        recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units, m, g, R, K, seed, level,
        fast=True)
    p = np.zeros(K, dtype=abi.SATURATION_POINT_DTYPE)
    for name in sr.POINT_KEYS:
        p[name] = [d[name] for d in pts]
    r = np.zeros(R, dtype=abi.SATURATION_PERM_DTYPE)
    for name in sr.PERM_KEYS:
        r[name] = [d[name] for d in perms]
    s = np.zeros(1, dtype=abi.SATURATION_SUMMARY_DTYPE)
    for name in sr.SUMMARY_KEYS:
        s[name] = summary[name]
    return (np.array(works, dtype=np.uint32), p, r, s,
            np.array(first, dtype=np.uint32).reshape(n_units, R))


def assert_equal(got, want):
    assert len(got) == len(want) == 5
    for a, b, dt in zip(got, want, DTYPES):
        a = np.asarray(a).reshape(-1)
        b = np.asarray(b).reshape(-1)
        assert len(a) == len(b), (len(a), len(b))
        if dt.names is None:
            bad = np.nonzero(a != b)[0]
            assert bad.size == 0, (int(bad[0]), a[bad[0]], b[bad[0]])
            continue
        for name in dt.names:                              # (the reserved words, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def last_times():
    ms = (C.c_double * 10)()
    assert _lib.load().fs_saturation_times(ms) == abi.FS_OK
    return dict(zip(abi.SATURATION_MS_NAMES, ms))


def check(index, monkeypatch, cols, n_works, unit_of, n_units, m=WIDTH, g=0, R=17, K=7, seed=0,
          level=95, paths=PATHS, want=None):
    """Both entry points down every path against the oracle; the host entry point's result."""
    from fandom_search_amd.engine import torch_ready
    if want is None:
        want = oracle(cols, n_works, unit_of, n_units, m, g, R, K, seed, level)
    d_rows, d_map = on_device(cols, unit_of)
    for env in paths:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        got = saturation.find_saturation(*cols, n_works, N_SCRIPT, unit_of, n_units, m, g, R, K,
                                         seed, level, first=True)
        assert_equal(got, want)
        torch_ready()
        dev = index.saturation_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                      n_units, m, g, R, K, seed, level, first=True)
        assert_equal(dev, want)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return got


def mixed(a, u):
    """Active work a quotes unit u: a bit of a product of both, so that the rows are all
    different and neither the matrix nor a block of it is symmetric."""
    return (((a + 1) * (2 * u + 3) * 2654435761) >> 13) & 1 == 1


def case(n_active, n_units, seed, rule=mixed, hole=True):
    """(cols, n_works, unit_of, inc): unit u owns the script words 3 u .. 3 u + 2; active work
    a quotes the units `rule` gives it, at least one (the last unit otherwise), each by a run of
    its own; with `hole` and more than one unit, nobody quotes the middle unit,
    (n_units - 1) // 2.  Works without a passage lie between the active ones, so the number of
    a work among all works and among the active ones differ.  inc[u][a] is the incidence over
    active numbers."""
    nobody = (n_units - 1) // 2 if hole and n_units > 1 else -1
    inc = np.zeros((n_units, n_active), dtype=np.int64)
    for a in range(n_active):
        mine = [u for u in range(n_units) if u != nobody and rule(a, u)] or [n_units - 1]
        inc[mine, a] = 1
    spans_of = interleaved(n_active, lambda k, rng: [
        (u * WIDTH, WIDTH) for u in np.nonzero(inc[:, k])[0].tolist()], seed=seed)
    unit_of = np.full(N_SCRIPT, NONE, dtype=np.uint32)
    unit_of[:n_units * WIDTH] = np.arange(n_units * WIDTH) // WIDTH
    return from_spans(spans_of), len(spans_of), unit_of, inc


def active_numbers(cols, m=WIDTH):
    """The work numbers of the active works of a case(): those with a run of m records."""
    work = cols[0]
    return np.array([w for w in np.unique(work).tolist() if (work == w).sum() >= m])


# ---- sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 129])
def test_active_works_around_a_word_of_the_rows(index, monkeypatch, n_active):
    cols, n_works, unit_of, inc = case(n_active, 17, seed=n_active)
    assert n_works > n_active                              # active numbers are not work numbers
    act = active_numbers(cols)
    assert len(act) == n_active and (n_active == 1 or (act != np.arange(n_active)).any())
    works, pts, perms, summary, first = check(index, monkeypatch, cols, n_works, unit_of, 17,
                                              seed=n_active)
    assert (works == inc.sum(axis=1)).all() and works[8] == 0
    assert int(summary["n_active"][0]) == n_active
    assert (pts["works_high"][-1], pts["works_sum"][-1]) == (n_works, 17 * n_works)
    assert (first[8] == NONE).all() and (first[works > 0] != NONE).all()


@pytest.mark.parametrize("n_units", [1, 63, 64, 65, 129])
def test_units_around_a_tile_and_a_curve_workgroup(index, monkeypatch, n_units):
    cols, n_works, unit_of, inc = case(65, n_units, seed=100 + n_units)
    works, pts, perms, summary, _ = check(index, monkeypatch, cols, n_works, unit_of, n_units,
                                          seed=5)
    assert (works == inc.sum(axis=1)).all() and works.sum() > 0
    Q = int((inc.sum(axis=1) > 0).sum())
    assert Q == int(summary["units_quoted"][0]) and 0 < Q <= n_units - (n_units > 1)
    assert n_units == 1 or works[(n_units - 1) // 2] == 0                  # the middle unit
    assert pts["units_median"][-1] == Q and pts["units_min"][-1] == Q      # S_r(K) = Q
    assert (perms["half_at"] <= perms["ninety_at"]).all()
    assert (perms["ninety_at"] <= perms["all_at"]).all()


@pytest.mark.parametrize("R", [1, 63, 64, 65, 130])
def test_orders_around_a_wave_of_lanes(index, monkeypatch, R):
    cols, n_works, unit_of, _ = case(65, 17, seed=200 + R)
    for level in (50, 95, 99):
        _, pts, perms, _, first = check(index, monkeypatch, cols, n_works, unit_of, 17, R=R,
                                        K=10, seed=R, level=level,
                                        paths=PATHS if level == 95 else PATHS[1:3])
        assert (pts["units_low"] <= pts["units_median"]).all()
        assert (pts["units_median"] <= pts["units_high"]).all()
    assert len(perms) == R and first.shape == (17, R)


def test_the_most_orders_the_sort_in_lds_takes(index, monkeypatch):
    cols, n_works, unit_of, _ = case(20, 5, seed=7)
    _, pts, perms, _, _ = check(index, monkeypatch, cols, n_works, unit_of, 5, R=4096, seed=11)
    assert len(perms) == 4096 and (pts["units_low"][:2] < pts["units_high"][:2]).all()
    assert last_times()["osplit"] == 64                    # two workgroups: a chunk to each wave
    assert (pts["works_low"][:6] < pts["works_high"][:6]).all()


@pytest.mark.parametrize("K", [1, 2, 7, 100, 1024])
def test_points_up_to_the_most(index, monkeypatch, K):
    cols, n_works, unit_of, inc = case(65, 17, seed=300 + K)
    _, pts, perms, summary, _ = check(index, monkeypatch, cols, n_works, unit_of, 17, R=33, K=K,
                                      seed=K, level=99 if K == 7 else 95)
    assert len(pts) == K and int(perms["all_at"].max()) <= K
    assert pts["units_max"][-1] == summary["units_quoted"][0] == (inc.sum(axis=1) > 0).sum() == 16
    for name in sr.POINT_KEYS:
        assert (np.diff(pts[name].astype(np.int64)) >= 0).all(), name


def test_the_words_of_a_row_shared_among_workgroups_by_default(index, monkeypatch):
    """1100 active works are 18 words; five product workgroups share them out by themselves,
    three parts of at least 8 words."""
    cols, n_works, unit_of, inc = case(1100, 17, seed=1400)
    works, _, _, _, _ = check(index, monkeypatch, cols, n_works, unit_of, 17, R=33, seed=4,
                              paths=[{}, {"FS_SATURATION_TABLE": "1"}])
    assert (works == inc.sum(axis=1)).all()
    assert last_times()["ksplit"] == 3 and last_times()["table"] == 1
    assert last_times()["osplit"] == 1                     # 33 orders are one chunk


# ---- content ----------------------------------------------------------------------------

def test_the_first_times_are_the_min_over_the_quoting_works(index, monkeypatch):
    """One order: first(0, u) is the smallest hash over the works of row u, by their numbers
    among all works; nothing else of the contract is looked at.  Neither the incidence nor the
    first times survive a swap of unit and work or of order and unit."""
    cols, n_works, unit_of, inc = case(129, 65, seed=31, hole=False)
    assert len({tuple(r) for r in inc.tolist()}) > 32 and (inc[:64, :64] != inc[:64, :64].T).any()
    for blk in (inc[:16, :16], inc[:65, :65]):
        assert (blk != blk.T).any()
    act = active_numbers(cols)
    assert len(act) == 129 and (act != np.arange(129)).any()
    for seed in (0, 9):
        h = sr.hash_np(seed, range(65), act)               # [order][active work]
        want = np.where(inc[:, None, :] == 1, h[None, :, :], NONE).min(axis=2)      # [u][r]
        assert (want != want.T).any() and (want < NONE).sum() > 32 * 65
        by_active_number = sr.hash_np(seed, range(65), range(129))
        assert (np.where(inc[:, None, :] == 1, by_active_number[None], NONE).min(axis=2)
                != want).any()
        for env in PATHS:
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            got = saturation.find_saturation(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0, 65,
                                             4, seed, 95, first=True)
            assert (got[4].astype(np.int64) == want).all(), env


def test_units_quoted_by_one_work_and_by_two(index, monkeypatch):
    # units 0 and 2: one work each; units 1 and 4: two, in one word of the row and in two; unit
    # 3: every work; unit 5: nobody
    def rule(a, u):
        return [a == 0, a in (1, 2), a == 3, True, a in (5, 70), False][u]
    cols, n_works, unit_of, _ = case(71, 6, seed=3, rule=rule, hole=False)
    works, pts, perms, summary, first = check(index, monkeypatch, cols, n_works, unit_of, 6,
                                              R=33, K=10, seed=2)
    assert works.tolist() == [1, 2, 1, 71, 2, 0]
    assert summary.tolist() == [(71, 5, 2, 2)]
    act = active_numbers(cols)
    assert first[0].tolist() == sr.hash_np(2, range(33), [act[0]])[:, 0].tolist()
    assert first[4].tolist() == sr.hash_np(2, range(33), [act[5], act[70]]).min(axis=1).tolist()
    assert (first[3] <= first[:5].min(axis=0)).all() and (first[5] == NONE).all()
    assert (perms["all_at"] >= perms["half_at"]).all() and pts["units_min"][-1] == 5


def test_works_are_those_of_intervals_and_the_curve_ends_at_the_quoted_units(index, monkeypatch):
    cols, n_works, unit_of, inc = case(129, 65, seed=41)
    works, pts, _, summary, _ = check(index, monkeypatch, cols, n_works, unit_of, 65, R=16,
                                      seed=1)
    theirs, _ = intervals.find_intervals(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0, 16, 1, 95)
    assert (works == theirs["works"]).all() and (works == inc.sum(axis=1)).all()
    Q = int(summary["units_quoted"][0])
    assert 32 < Q == int((works > 0).sum()) == int(pts["units_median"][-1]) < 65
    assert int(summary["singletons"][0]) == int((works == 1).sum())
    assert int(summary["doubletons"][0]) == int((works == 2).sum())
    ms = last_times()
    assert ms["product"] > 0 and abs(ms["total"] - sum(list(ms.values())[:6])) < 1e-9


# ---- the byte limit -----------------------------------------------------------------------

def test_the_byte_limit_drops_the_table_and_then_refuses(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    cols, n_works, unit_of, _ = case(65, 17, seed=9)
    want = oracle(cols, n_works, unit_of, 17, WIDTH, 0, 17, 7, 0, 95)
    table_on = [{"FS_SATURATION_TABLE": "1", "FS_SATURATION_KSPLIT": "1"}]
    # 65 active works, 17 units, 17 orders padded to 64, 7 points: a matrix of 64 x 2 x 8 bytes,
    # first times of 17 x 64 x 4, histograms of 2 x 7 x 64 x 4, a table of 65 x 64 x 4
    mat, first, hist, table = 1024, 4352, 3584, 16640
    monkeypatch.setenv("FS_SATURATION_MAX_BYTES", str(mat + first + hist + table))
    check(index, monkeypatch, cols, n_works, unit_of, 17, paths=table_on, want=want)
    assert last_times()["table"] == 1                      # at the bound: the table is read
    monkeypatch.setenv("FS_SATURATION_MAX_BYTES", str(mat + first + hist + table - 1))
    check(index, monkeypatch, cols, n_works, unit_of, 17, paths=table_on, want=want)
    assert last_times()["table"] == 0                      # one byte less: hashed in the lane
    monkeypatch.setenv("FS_SATURATION_MAX_BYTES", str(mat + first + hist))
    check(index, monkeypatch, cols, n_works, unit_of, 17, paths=table_on, want=want)
    assert last_times()["table"] == 0
    monkeypatch.setenv("FS_SATURATION_MAX_BYTES", str(mat + first + hist - 1))
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    for call in (lambda: saturation.find_saturation(*cols, n_works, N_SCRIPT, unit_of, 17, WIDTH,
                                                    0, 17, 7),
                 lambda: index.saturation_device(d_rows.data_ptr(), len(cols[0]), n_works,
                                                 d_map.data_ptr(), 17, WIDTH, 0, 17, 7)):
        with pytest.raises(_lib.FsError) as e:
            call()
        assert e.value.code == abi.FS_E_UNSUPPORTED
        text = str(e.value)
        assert "17 units over 65 works with a passage in 17 orders and 7 points" in text
        assert "an incidence matrix of 1024 bytes" in text
        assert "first times of 4352 bytes" in text and "histograms of 3584 bytes" in text
        assert "more than 8959 bytes" in text
    monkeypatch.delenv("FS_SATURATION_MAX_BYTES")


# ---- errors and edges -------------------------------------------------------------------

def test_no_records_no_units_and_no_active_work(index, monkeypatch):
    empty = (np.zeros(0, np.uint32),) * 3
    cols, n_works, unit_of, _ = case(10, 5, seed=2)
    works, pts, perms, summary, first = check(index, monkeypatch, empty, 3, unit_of, 5, R=16)
    assert not works.any() and (first == NONE).all() and first.shape == (5, 16)
    assert perms.tolist() == [(1, 1, 1, 0)] * 16 and summary.tolist() == [(0, 0, 0, 0)]
    assert not pts["units_max"].any() and pts["works_low"][-1] == 3 and pts["works_sum"][-1] == 48
    got = check(index, monkeypatch, cols, n_works, np.full(N_SCRIPT, NONE, np.uint32), 0)
    assert len(got[0]) == 0 and got[4].size == 0 and int(got[3]["n_active"][0]) == 10
    assert got[2].tolist() == [(1, 1, 1, 0)] * 17
    works, pts, perms, summary, first = check(index, monkeypatch, cols, n_works, unit_of, 5, m=4)
    assert not works.any() and summary.tolist() == [(0, 0, 0, 0)]          # no passage
    assert pts["works_median"][-1] == n_works and (first == NONE).all()


def test_refusals(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    cols, n_works, unit_of, _ = case(65, 17, seed=9)

    def refused(c=cols, n_works=n_works, unit_of=unit_of, n_units=17, m=WIDTH, R=17, K=7,
                level=95, code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            saturation.find_saturation(*c, n_works, N_SCRIPT, unit_of, n_units, m, 0, R, K, 0,
                                       level)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.saturation_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                    n_units, m, 0, R, K, 0, level)
        assert e.value.code == code
        return str(e.value)
    refused(m=0)
    assert "permutations 0: from 1 to 4096" in refused(R=0)
    refused(R=4097)
    refused(K=0)
    assert "points 1025: from 1 to 1024" in refused(K=1025)
    refused(level=49)
    refused(level=100)
    refused(n_works=int(cols[0].max()))                    # a work >= n_works
    # and without a unit the records are checked all the same: one work, eight records, the last
    # of a work >= n_works
    stray = (np.array([0] * 7 + [1], np.uint32), np.arange(8, dtype=np.uint32),
             np.arange(10, 18, dtype=np.uint32))
    text = refused(stray, n_works=1, unit_of=np.full(N_SCRIPT, NONE, np.uint32), n_units=0, m=3)
    assert "a work >= n_works or an orig_ix >= n_script" in text
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # an orig_ix >= n_script
    fan = cols[1].copy()
    at = int(np.nonzero(cols[0] == active_numbers(cols)[0])[0][0])
    fan[at], fan[at + 1] = fan[at + 1], fan[at]
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    bad = unit_of.copy()
    bad[N_SCRIPT - 1] = 17                                 # neither below n_units nor none
    assert "neither below n_units (17) nor 0xFFFFFFFF" in refused(unit_of=bad)


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case_,by,m,g,k,R,K,seed,level", msg.CASES)
def test_command_on_the_golden_input(tmp_path, case_, by, m, g, k, R, K, seed, level, reader):
    src = os.path.join(GOLDEN, msg.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["saturation", src, "-o", prefix, "--by", by, "--min-words", str(m),
                 "--max-gap", str(g), "--min-works", str(k), "--permutations", str(R),
                 "--points", str(K), "--seed", str(seed), "--level", str(level),
                 "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in saturation.output_names(src, prefix))
    for name, part in zip(msg.golden_names(case_), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_by_default_the_default_prefix_and_a_file_without_records(tmp_path):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, msg.INPUT), src)
    assert main(["saturation", src]) == 0                  # every default: the first golden
    for path, name in zip(saturation.output_names(src), msg.golden_names("default")):
        with open(path, "rb") as fh, open(os.path.join(GOLDEN, name), "rb") as want:
            assert fh.read() == want.read(), path
    assert main(["saturation", src, "--by", "character", "--permutations", "20", "--points", "5",
                 "--seed", "3"]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        want = sr.saturation_csv(fh.read(), "character", permutations=20, points=5, seed=3)
    for path, text in zip(saturation.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert [t.count("\r\n") for t in want] == [6, 21, 2]
    with open(src, "w", newline="", encoding="utf-8") as fh:
        fh.write(open(os.path.join(GOLDEN, msg.INPUT), newline="").readline())
    for reader in ("device", "python"):
        assert main(["saturation", src, "--reader", reader]) == 0
        for path, head in zip(saturation.output_names(src),
                              (sr.POINT_FIELDS, sr.PERMUTATION_FIELDS, sr.SUMMARY_FIELDS)):
            with open(path, "rb") as fh:
                assert fh.read() == (",".join(head) + "\r\n").encode("utf-8")
