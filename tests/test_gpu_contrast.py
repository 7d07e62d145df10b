"""`contrast` on the GPU: fs_contrast and fs_contrast_rows against the restated contract
(tests/contrast_restated.py), every field of both records and the whole table of a_r(u) compared
for equality; pools, sides, keys, active works, units and permutations around every size the
kernels treat differently; an incidence that no swap of row and column in a map leaves
unchanged; `ao3.py contrast` byte for byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, companions, contrast, intervals, synth
from fandom_search_amd.cli import main
from tests import contrast_restated as cn
from tests.golden import make_contrast_golden as mcg
from tests.test_gpu_companions import on_device
from tests.test_gpu_intervals import N_SCRIPT, WIDTH, active_numbers, case, mixed, quoted

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, side, m, g, q, P, seed, bits, fast=False):
    recs = list(zip(*(c.tolist() for c in cols)))
    units, perms, a_r = cn.contrast(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(),
                                    n_units, np.asarray(side).tolist(), m, g, q, P, seed, bits,
                                    fast=fast)
    u = np.zeros(n_units, dtype=abi.CONTRAST_UNIT_DTYPE)
    for name in cn.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    p = np.zeros(P, dtype=abi.CONTRAST_PERM_DTYPE)
    for name in cn.PERM_KEYS:
        p[name] = [d[name] for d in perms]
    return u, p, np.array(a_r, dtype=np.uint32).reshape(n_units, P)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.CONTRAST_UNIT_DTYPE, abi.CONTRAST_PERM_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])
    if len(got) > 2:
        bad = np.argwhere(got[2] != want[2])
        assert bad.size == 0, ("a_counts", bad[0].tolist(), got[2][tuple(bad[0])],
                               want[2][tuple(bad[0])])


def check(index, cols, n_works, unit_of, n_units, side, m=WIDTH, g=0, q=1, P=17, seed=0,
          bits=32, device=True, fast=False):
    """Both entry points against the oracle; the host entry point's result."""
    from fandom_search_amd.engine import torch_ready
    import torch
    want = oracle(cols, n_works, unit_of, n_units, side, m, g, q, P, seed, bits, fast)
    got = contrast.find_contrast(*cols, n_works, N_SCRIPT, unit_of, n_units, side, m, g, q, P,
                                 seed, bits, a_counts=True)
    assert_equal(got, want)
    if device:
        d_rows, d_map = on_device(cols, unit_of)
        d_side = torch.from_numpy(np.ascontiguousarray(side, dtype=np.uint8)
                                  if len(side) else np.zeros(1, np.uint8)).to("cuda")
        torch_ready()
        dev = index.contrast_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                    n_units, d_side.data_ptr(), m, g, q, P, seed, bits)
        assert_equal(dev, want[:2])
    return got


def sides(n_works, pool, na, seed):
    """Side bytes with every third work out of the pool: the first `pool` of the others are in
    it, `na` of them, picked by a shuffle, on side A."""
    inside = [w for w in range(n_works) if w % 3 != 2][:pool]
    assert len(inside) == pool, (n_works, pool)
    side = np.zeros(n_works, dtype=np.uint8)
    side[inside] = 2
    side[np.random.default_rng(seed).permutation(inside)[:na]] = 1
    return side


# ---- selection --------------------------------------------------------------------------

@pytest.mark.parametrize("pool", [2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_pools_sides_keys_and_permutations(index, pool):
    """Pool position, work number and active number all differ: works without a passage lie
    between the active ones, and every third work is out of the pool."""
    cols, n_works, unit_of, inc = case(max(4, pool), 5, seed=pool)
    assert n_works * 2 // 3 >= pool
    combos = [(na, bits, P) for na in sorted({1, pool // 2, pool - 1})
              for bits in (32, 4, 0) for P in (1, 2, 65)]
    for k, (na, bits, P) in enumerate(combos):
        side = sides(n_works, pool, na, seed=k)
        units, perms, counts = check(index, cols, n_works, unit_of, 5, side, P=P, seed=k,
                                     bits=bits)
        assert len(perms) == P and counts.shape == (5, P)
        if bits == 0:                                      # the first NA pool works, every time
            assert (counts == counts[:, :1]).all()


def test_ties_at_the_boundary_are_the_rule_at_four_bits(index):
    cols, n_works, unit_of, _ = case(257, 5, seed=77)
    side = sides(n_works, 300, 150, seed=1)
    pool = np.nonzero(side)[0]
    for r in range(3):
        keys = cn.keys_np(5, r, pool, 4)
        kth = np.sort(keys)[149]
        assert (keys == kth).sum() > 5                     # many works at the boundary key
    check(index, cols, n_works, unit_of, 5, side, P=3, seed=5, bits=4)


# ---- product ----------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("n_units", [1, 63, 64, 65])
def test_active_works_and_units_around_a_word_and_a_tile(index, n_active, n_units):
    cols, n_works, unit_of, inc = case(n_active, n_units, seed=n_active + n_units, rule=mixed)
    assert n_works > n_active
    pool = n_works * 2 // 3
    side = sides(n_works, pool, max(1, pool // 3), seed=n_units)
    units, _, counts = check(index, cols, n_works, unit_of, n_units, side, P=9, seed=n_active)
    act = active_numbers(cols)
    assert ((units["a_works"] + units["b_works"]) == inc[:, side[act] != 0].sum(axis=1)).all()


@pytest.mark.parametrize("P", [61, 62, 63, 64])
def test_permutations_around_a_tile_of_rows_with_the_two_observed_ones(index, P):
    cols, n_works, unit_of, _ = case(129, 65, seed=P, rule=mixed)
    side = sides(n_works, n_works * 2 // 3, n_works // 4, seed=P)
    _, perms, counts = check(index, cols, n_works, unit_of, 65, side, q=3, P=P, seed=P)
    assert counts.shape == (65, P) and len(set(perms["max_statistic"].tolist())) > 5


def test_the_most_permutations(index):
    cols, n_works, unit_of, _ = case(20, 5, seed=7)
    side = sides(n_works, n_works * 2 // 3, 7, seed=3)
    units, perms, _ = check(index, cols, n_works, unit_of, 5, side, q=2, P=4096, seed=11)
    assert len(perms) == 4096 and (units["ge"] > 0).any()


# ---- the incidence and the label layout ----------------------------------------------------

def test_one_unit_per_active_work_reads_the_label_bits_themselves(index):
    """a_r(u) is the label of active work u in permutation r: a swap of row and column in the
    map of L, of M or of the counts changes a count."""
    n = 70
    cols, n_works, unit_of, inc = case(n, n, seed=5, rule=lambda a, u: a == u)
    assert (inc == np.eye(n, dtype=np.int64)).all()
    side = sides(n_works, n_works * 2 // 3, n_works // 3, seed=2)
    act = active_numbers(cols)
    for bits in (32, 4):
        units, perms, counts = check(index, cols, n_works, unit_of, n, side, P=70, seed=3,
                                     bits=bits)
        assert counts.max() == 1 and (counts != counts.T).any()
        sets = cn.drawn(side.tolist(), 70, 3, bits)
        want = np.array([[int(act[u]) in sets[r] for r in range(70)] for u in range(n)])
        assert (counts == want).all()
        assert (perms["a_active"] == counts.sum(axis=0)).all()


def test_an_incidence_that_is_not_symmetric(index):
    cols, n_works, unit_of, inc = case(129, 65, seed=31, rule=mixed)
    assert len({tuple(r) for r in inc.tolist()}) == 65 and (inc[:64, :64] != inc[:64, :64].T).any()
    side = sides(n_works, n_works * 2 // 3, n_works // 3, seed=4)
    _, _, counts = check(index, cols, n_works, unit_of, 65, side, q=5, P=66, seed=9)
    act = active_numbers(cols)
    sets = cn.drawn(side.tolist(), 66, 9, 32)
    lab = np.array([[int(w) in sets[r] for w in act] for r in range(66)], dtype=np.int64)
    assert (counts == inc @ lab.T).all() and (lab[:64, :64] != lab[:64, :64].T).any()
    cols, n_works, unit_of, _ = case(64, 64, seed=8, rule=quoted)
    check(index, cols, n_works, unit_of, 64, sides(n_works, n_works * 2 // 3, 9, seed=1), P=64)


# ---- family and degenerate units ---------------------------------------------------------

def test_family_ties_and_degenerate_units(index):
    # units 0 and 3: the same works (bit 0 of a); unit 1: nobody; unit 2: every active work;
    # units 4 and 5: different works, as many
    def rule(a, u):
        return [a & 1, 0, 1, a & 1, a & 2, a & 4][u] != 0
    cols, n_works, unit_of, inc = case(64, 6, seed=3, rule=rule)
    act = active_numbers(cols)
    side = np.zeros(n_works, dtype=np.uint8)               # the pool: the active works alone
    side[act] = 2
    side[act[(act * 7) % 5 < 2]] = 1
    units, perms, _ = check(index, cols, n_works, unit_of, 6, side, q=1, P=33, seed=2)
    assert (units["a_works"] + units["b_works"]).tolist() == [32, 0, 64, 32, 32, 32]
    assert tuple(units[1]) == (0, 0, 33, NONE, 0, 0)       # nobody quotes it: outside the family
    assert tuple(units[2])[2:] == (33, 33, 0, 0)           # every pool work: den = 0, in it
    assert tuple(units[0]) == tuple(units[3])
    assert 3 not in perms["max_unit"].tolist() and 0 in perms["max_unit"].tolist()
    # min_quoting exactly at t(u) and one above it
    units, _, _ = check(index, cols, n_works, unit_of, 6, side, q=32, P=33, seed=2)
    assert (units["adj_ge"] != NONE).tolist() == [True, False, True, True, True, True]
    units, perms, _ = check(index, cols, n_works, unit_of, 6, side, q=33, P=33, seed=2)
    assert (units["adj_ge"] != NONE).tolist() == [False, False, True, False, False, False]
    assert not perms["max_statistic"].any() and (perms["max_unit"] == 2).all()
    # an empty family
    units, perms, _ = check(index, cols, n_works, unit_of, 6, side, q=65, P=33, seed=2)
    assert (units["adj_ge"] == NONE).all() and (perms["max_unit"] == NONE).all()
    assert not perms["max_statistic"].any() and perms["a_active"].all()


def test_no_pool_work_active_no_records_no_units_and_an_empty_side(index):
    cols, n_works, unit_of, _ = case(10, 5, seed=2)
    act = active_numbers(cols)
    side = np.full(n_works, 2, dtype=np.uint8)
    side[::2] = 1
    side[act] = 0                                          # every active work out of the pool
    assert (side == 1).any() and (side == 2).any()
    units, perms, counts = check(index, cols, n_works, unit_of, 5, side, P=16)
    assert not counts.any() and (units["ge"] == 16).all() and (units["adj_ge"] == NONE).all()
    assert not perms["a_active"].any() and (perms["max_unit"] == NONE).all()
    side = sides(n_works, n_works * 2 // 3, 3, seed=1)
    empty = (np.zeros(0, np.uint32),) * 3
    units, perms, counts = check(index, empty, n_works, unit_of, 5, side, P=16)
    assert (units["ge"] == 16).all() and not counts.any() and not perms["a_active"].any()
    units, perms, counts = check(index, cols, n_works, np.full(N_SCRIPT, NONE, np.uint32), 0,
                                 side, P=16)
    assert len(units) == 0 and counts.shape == (0, 16) and perms["a_active"].any()
    check(index, cols, n_works, unit_of, 5, side, m=4, P=16)          # no passage
    for one in (1, 2):                                                # an empty side
        units, perms, _ = check(index, cols, n_works, unit_of, 5,
                                np.where(side != 0, one, 0).astype(np.uint8), P=16)
        assert not units["d"].any() and (units["ge"] == 16).all()
        assert perms["a_active"].any() == (one == 1)
    check(index, cols, n_works, unit_of, 5, np.zeros(n_works, np.uint8), P=16)   # an empty pool


# ---- 64-bit arithmetic and the bound -----------------------------------------------------

def test_a_million_works(index):
    """n_works at the bound: |D| << 20 needs more than 32 bits many times over, and the
    selection's histograms hold hundreds of works per bin."""
    n_works = 1 << 20
    cols, small, unit_of, inc = case(40, 5, seed=12)
    act = active_numbers(cols)
    spread = np.zeros(small, dtype=np.int64)               # the works of the case, far apart
    spread[:] = np.arange(small) * ((n_works - 1) // (small - 1))
    assert spread[-1] == n_works - 1 or spread[-1] < n_works
    spread[-1] = n_works - 1
    cols = (spread[cols[0]].astype(np.uint32), cols[1], cols[2])
    side = np.full(n_works, 2, dtype=np.uint8)
    side[2::3] = 0
    side[np.arange(0, n_works, 7)] = 1
    side[spread[act[::2]]] = 1
    side[spread[act[1::4]]] = 2
    units, perms, _ = check(index, cols, n_works, unit_of, 5, side, q=2, P=2, seed=3,
                            device=False, fast=True)
    n = int((side != 0).sum())
    assert n > 600000 and int(np.abs(units["d"]).max()) << 20 > 1 << 40
    assert (units["statistic"] > 1 << 20).any()


# ---- switches and cross-checks -----------------------------------------------------------

def test_every_atomic_issued_gives_the_same_records(index, monkeypatch):
    cols, n_works, unit_of, _ = case(129, 65, seed=41, rule=mixed)
    side = sides(n_works, n_works * 2 // 3, n_works // 3, seed=6)
    first = check(index, cols, n_works, unit_of, 65, side, q=4, P=130, seed=1)
    monkeypatch.setenv("FS_CONTRAST_PRECHECK", "0")
    second = check(index, cols, n_works, unit_of, 65, side, q=4, P=130, seed=1)
    monkeypatch.delenv("FS_CONTRAST_PRECHECK")
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    L = _lib.load()
    ms = (C.c_double * 5)()
    assert L.fs_contrast_times(ms) == abi.FS_OK
    assert ms[1] > 0 and ms[2] > 0 and abs(ms[4] - sum(ms[:4])) < 1e-9


def test_the_two_sides_add_up_to_the_works_of_intervals_and_companions(index):
    cols, n_works, unit_of, _ = case(129, 65, seed=41, rule=mixed)
    side = np.where(np.arange(n_works) % 3 == 0, 1, 2).astype(np.uint8)     # every work in the pool
    units, _, _ = check(index, cols, n_works, unit_of, 65, side, P=16, seed=1)
    theirs, _ = companions.find_companions(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0, 2, 0)
    assert ((units["a_works"] + units["b_works"]) == theirs["works"]).all()
    again, _ = intervals.find_intervals(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0, 16, 1, 95)
    assert ((units["a_works"] + units["b_works"]) == again["works"]).all()
    assert (units["a_works"] > 0).sum() >= 60


def test_two_seeds_differ_and_one_seed_repeats(index):
    cols, n_works, unit_of, _ = case(65, 17, seed=9)
    side = sides(n_works, n_works * 2 // 3, n_works // 3, seed=6)
    one = check(index, cols, n_works, unit_of, 17, side, P=33, seed=1)
    same = check(index, cols, n_works, unit_of, 17, side, P=33, seed=1)
    other = check(index, cols, n_works, unit_of, 17, side, P=33, seed=2)
    for a, b in zip(one, same):
        assert a.tobytes() == b.tobytes()
    assert (one[2] != other[2]).any() and one[0]["d"].tolist() == other[0]["d"].tolist()


# ---- refusals -----------------------------------------------------------------------------

def test_refusals_and_the_size_cap(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    import torch
    cols, n_works, unit_of, _ = case(65, 17, seed=9)
    good = sides(n_works, n_works * 2 // 3, n_works // 3, seed=6)

    def refused(c=cols, n_works=n_works, unit_of=unit_of, n_units=17, side=good, m=WIDTH, q=1,
                P=17, bits=32, code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            contrast.find_contrast(*c, n_works, N_SCRIPT, unit_of, n_units, side[:n_works], m, 0,
                                   q, P, 0, bits)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        d_side = torch.from_numpy(np.ascontiguousarray(side)).to("cuda")
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.contrast_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                  n_units, d_side.data_ptr(), m, 0, q, P, 0, bits)
        assert e.value.code == code
        return str(e.value)
    refused(m=0)
    refused(q=0)
    refused(P=0)
    refused(P=4097)
    refused(bits=33)
    three = good.copy()
    three[n_works - 1] = 3
    assert "side byte" in refused(side=three)
    refused(n_works=int(cols[0].max()))                    # a work >= n_works
    # and without a unit the records are checked all the same: one work, eight records, the last
    # of a work >= n_works
    stray = (np.array([0] * 7 + [1], np.uint32), np.arange(8, dtype=np.uint32),
             np.arange(10, 18, dtype=np.uint32))
    text = refused(stray, n_works=1, unit_of=np.full(N_SCRIPT, NONE, np.uint32), n_units=0,
                   side=np.ones(1, np.uint8), m=3)
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
    refused(unit_of=bad)
    # n_works above the bound: refused before a byte of side is read
    with pytest.raises(_lib.FsError) as e:
        contrast.find_contrast(*cols, (1 << 20) + 1, N_SCRIPT, unit_of, 17,
                               np.zeros((1 << 20) + 1, np.uint8), WIDTH, 0, 1, 17, 0, 32)
    assert e.value.code == abi.FS_E_UNSUPPORTED
    # 65 active works: a matrix of 64 x 2 x 8 bytes, 64 x 2 x 8 label bytes, 64 x 64 counts
    monkeypatch.setenv("FS_CONTRAST_MAX_BYTES", str(1024 + 1024 + 16384 - 1))
    text = refused(code=abi.FS_E_UNSUPPORTED)
    assert "an incidence matrix of 1024 bytes" in text
    assert "labels of 1024 bytes" in text and "counts of 16384 bytes" in text
    assert "more than 18431 bytes" in text
    monkeypatch.setenv("FS_CONTRAST_MAX_BYTES", str(1024 + 1024 + 16384))
    check(index, cols, n_works, unit_of, 17, good)         # at the bound: accepted
    monkeypatch.delenv("FS_CONTRAST_MAX_BYTES")


# ---- the command ------------------------------------------------------------------------

def command(src, meta, by, a_keys, b_keys, unit, m, g, k, q, P, seed, more=()):
    argv = ["contrast", src, meta, "--by", by, "--unit", unit, "--min-words", str(m),
            "--max-gap", str(g), "--min-works", str(k), "--min-quoting", str(q),
            "--permutations", str(P), "--seed", str(seed)]
    for key in a_keys:
        argv += ["--a", key]
    for key in b_keys:
        argv += ["--b", key]
    return main(argv + list(more))


@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case_,by,a_keys,b_keys,unit,m,g,k,q,P,seed", mcg.CASES)
def test_command_on_the_golden_input(tmp_path, case_, by, a_keys, b_keys, unit, m, g, k, q, P,
                                     seed, reader):
    src, meta = os.path.join(GOLDEN, mcg.INPUT), os.path.join(GOLDEN, mcg.META)
    prefix = str(tmp_path / "p")
    assert command(src, meta, by, a_keys, b_keys, unit, m, g, k, q, P, seed,
                   ["-o", prefix, "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in contrast.output_names(src, prefix))
    for name, part in zip(mcg.golden_names(case_), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_the_default_prefix_and_a_file_without_records(tmp_path):
    import shutil
    src, meta = str(tmp_path / "m.csv"), os.path.join(GOLDEN, mcg.META)
    shutil.copy(os.path.join(GOLDEN, mcg.INPUT), src)
    assert main(["contrast", src, meta, "--by", "language", "--a", "Deutsch", "--b", "English",
                 "--unit", "character", "--permutations", "20", "--seed", "3",
                 "--min-quoting", "2"]) == 0
    with open(src, newline="", encoding="utf-8") as fh, \
            open(meta, newline="", encoding="utf-8") as mh:
        want = cn.contrast_csv(fh.read(), mh.read(), "language", ("Deutsch",), ("English",),
                               "character", min_quoting=2, permutations=20, seed=3)
    for path, text in zip(contrast.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[1].count("\r\n") == 5 and want[2].count("\r\n") == 21
    assert want[1].splitlines()[4].startswith("OUT,,") and not want[1].startswith("OUT,,0")
    with pytest.raises(SystemExit) as e:
        main(["contrast", src, meta, "--by", "language", "--a", "Klingon"])
    assert str(e.value.code) == ("ao3.py contrast: error: side A is empty: no work of the match "
                                 "file has one of its keys")
    with open(src, "w", newline="", encoding="utf-8") as fh:
        fh.write(open(os.path.join(GOLDEN, mcg.INPUT), newline="").readline())
    for reader in ("device", "python"):
        assert main(["contrast", src, meta, "--a", "2016", "--reader", reader]) == 0
        for path, head in zip(contrast.output_names(src),
                              (cn.UNIT_FIELDS, cn.SIDE_FIELDS, cn.PERMUTATION_FIELDS)):
            with open(path, "rb") as fh:
                assert fh.read() == (",".join(head) + "\r\n").encode("utf-8")
