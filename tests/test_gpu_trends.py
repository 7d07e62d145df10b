"""`trends` on the GPU: fs_trends and fs_trends_rows against the restated contract
(tests/trends_restated.py), every field of both records and the whole table of s_r(u) compared
for equality, with the product by MFMA (FS_TRENDS_MFMA unset) and by the plain kernel (0);
active works, units and re-datings around every size the kernels treat differently; pools with
works outside and inactive works inside; offsets at the edge of the two byte planes; an
incidence that no swap of row and column in a fragment map leaves unchanged; `ao3.py trends`
byte for byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, trends
from fandom_search_amd.cli import main
from tests import trends_restated as tr
from tests.golden import make_trends_golden as mtg
from tests.test_gpu_companions import on_device
from tests.test_gpu_intervals import N_SCRIPT, WIDTH, active_numbers, case, mixed, quoted

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
OUT = abi.TRENDS_OUT


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd import synth
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, when, m, g, q, P, seed, fast=False):
    recs = list(zip(*(c.tolist() for c in cols)))
    units, perms, s_r = tr.trends(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units,
                                  np.asarray(when).tolist(), m, g, q, P, seed, fast=fast)
    u = np.zeros(n_units, dtype=abi.TRENDS_UNIT_DTYPE)
    for name in tr.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    p = np.zeros(P, dtype=abi.TRENDS_PERM_DTYPE)
    for name in tr.PERM_KEYS:
        p[name] = [d[name] for d in perms]
    return u, p, np.array(s_r, dtype=np.uint32).reshape(n_units, P)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.TRENDS_UNIT_DTYPE, abi.TRENDS_PERM_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])
    if len(got) > 2:
        bad = np.argwhere(got[2] != want[2])
        assert bad.size == 0, ("sums", bad[0].tolist(), got[2][tuple(bad[0])],
                               want[2][tuple(bad[0])])


def check(index, monkeypatch, cols, n_works, unit_of, n_units, when, m=WIDTH, g=0, q=1, P=17,
          seed=0, device=True, fast=False, products=(None, "0")):
    """Both entry points under both products against the oracle; the host entry point's
    result."""
    from fandom_search_amd.engine import torch_ready
    import torch
    want = oracle(cols, n_works, unit_of, n_units, when, m, g, q, P, seed, fast)
    when = np.ascontiguousarray(when, dtype=np.uint16)
    for mfma in products:
        if mfma is None:
            monkeypatch.delenv("FS_TRENDS_MFMA", raising=False)
        else:
            monkeypatch.setenv("FS_TRENDS_MFMA", mfma)
        got = trends.find_trends(*cols, n_works, N_SCRIPT, unit_of, n_units, when, m, g, q, P,
                                 seed, sums=True)
        assert_equal(got, want)
        if device:
            d_rows, d_map = on_device(cols, unit_of)
            d_when = torch.from_numpy(when.view(np.int16) if len(when)
                                      else np.zeros(1, np.int16)).to("cuda")
            torch_ready()
            dev = index.trends_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                      n_units, d_when.data_ptr(), m, g, q, P, seed)
            assert_equal(dev, want[:2])
    monkeypatch.delenv("FS_TRENDS_MFMA", raising=False)
    return got


def dates(n_works, seed, span=240, out=True):
    """A period offset per work, below `span`; every third work outside the pool."""
    when = np.random.default_rng(seed).integers(0, span, n_works).astype(np.uint16)
    if out:
        when[2::3] = OUT
    return when


# ---- sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("n_units", [1, 15, 16, 17, 65])
def test_active_works_and_units_around_a_word_a_fragment_and_a_tile(index, monkeypatch, n_active,
                                                                    n_units):
    """Pool position, work number and active number all differ: works without a passage lie
    between the active ones and are in the pool, and every third work is outside it."""
    cols, n_works, unit_of, inc = case(n_active, n_units, seed=n_active + n_units, rule=mixed)
    assert n_works > n_active
    when = dates(n_works, seed=n_units)
    units, perms, sums = check(index, monkeypatch, cols, n_works, unit_of, n_units, when, P=9,
                               seed=n_active)
    act = active_numbers(cols)
    assert (units["quoting"] == inc[:, when[act] != OUT].sum(axis=1)).all()
    inactive = np.setdiff1d(np.arange(n_works), act)
    assert n_works < 3 or (when[inactive] != OUT).any()
    assert sums.shape == (n_units, 9)


@pytest.mark.parametrize("P", [1, 15, 16, 17, 64])
def test_redatings_around_a_fragment_with_the_observed_row_behind_them(index, monkeypatch, P):
    cols, n_works, unit_of, _ = case(65, 17, seed=P, rule=mixed)
    when = dates(n_works, seed=P)
    _, perms, sums = check(index, monkeypatch, cols, n_works, unit_of, 17, when, q=3, P=P, seed=P)
    assert sums.shape == (17, P) and len(perms) == P


def test_the_most_redatings(index, monkeypatch):
    cols, n_works, unit_of, _ = case(20, 5, seed=7)
    when = dates(n_works, seed=3, span=1024)
    units, perms, _ = check(index, monkeypatch, cols, n_works, unit_of, 5, when, q=2, P=4096,
                            seed=11)
    assert len(perms) == 4096 and (units["ge"] > 0).any()
    assert len(set(perms["offset_sum"].tolist())) > 100    # X_r varies: drawn with replacement


# ---- the two planes -------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["all 127", "all 128", "0 and one 1023", "every value"])
def test_offsets_at_the_edge_of_the_planes(index, monkeypatch, kind):
    cols, n_works, unit_of, _ = case(65, 17, seed=21, rule=mixed)
    act = active_numbers(cols)
    if kind == "every value":
        when = (np.arange(n_works) * 41 % 1024).astype(np.uint16)
    else:
        when = np.full(n_works, {"all 127": 127, "all 128": 128}.get(kind, 0), dtype=np.uint16)
        if kind == "0 and one 1023":
            when[act[3]] = 1023
    units, perms, sums = check(index, monkeypatch, cols, n_works, unit_of, 17, when, P=33, seed=5)
    if kind in ("all 127", "all 128"):                       # one period: nothing moves
        assert not units["d"].any() and (units["ge"] == 33).all()
        assert (sums == units["quoting"][:, None] * int(when[0])).all()
    if kind == "0 and one 1023":
        assert set(np.unique(sums).tolist()) - {0, 1023} and (sums % 1023 == 0).all()
        assert (units["last_x"][units["quoting"] > 0] % 1023 == 0).all()


# ---- the incidence and the label layout ----------------------------------------------------

def labels_of(when, act, P, seed):
    x_r = tr.redated(np.asarray(when).tolist(), P, seed)
    return np.array([[x_r[r][int(w)] for w in act] for r in range(P)], dtype=np.int64)


def test_one_unit_per_active_work_reads_the_labels_themselves(index, monkeypatch):
    """s_r(u) is the offset of active work u in re-dating r: a swap of row and column in the
    map of a plane, of M or of the sums changes one."""
    n = 70
    cols, n_works, unit_of, inc = case(n, n, seed=5, rule=lambda a, u: a == u)
    assert (inc == np.eye(n, dtype=np.int64)).all()
    when = dates(n_works, seed=2, span=1024)
    act = active_numbers(cols)
    units, perms, sums = check(index, monkeypatch, cols, n_works, unit_of, n, when, P=70, seed=3)
    want = labels_of(when, act, 70, 3).T
    assert (sums == want).all() and (sums != sums.T).any() and sums.max() > 127
    assert (units["offset_sum"] == np.where(when[act] == OUT, 0, when[act])).all()


def test_an_incidence_that_is_not_symmetric(index, monkeypatch):
    cols, n_works, unit_of, inc = case(129, 65, seed=31, rule=mixed)
    assert len({tuple(r) for r in inc.tolist()}) == 65 and (inc[:64, :64] != inc[:64, :64].T).any()
    when = dates(n_works, seed=4, span=1024)
    _, _, sums = check(index, monkeypatch, cols, n_works, unit_of, 65, when, q=5, P=66, seed=9)
    lab = labels_of(when, active_numbers(cols), 66, 9)
    assert (sums == inc @ lab.T).all() and (lab[:64, :64] != lab[:64, :64].T).any()
    cols, n_works, unit_of, _ = case(64, 64, seed=8, rule=quoted)
    check(index, monkeypatch, cols, n_works, unit_of, 64, dates(n_works, seed=1), P=64)


def test_the_words_of_a_tile_shared_among_workgroups(index, monkeypatch):
    cols, n_works, unit_of, _ = case(257, 17, seed=13, rule=mixed)
    when = dates(n_works, seed=6, span=1024)
    first = check(index, monkeypatch, cols, n_works, unit_of, 17, when, q=4, P=33, seed=1,
                  products=(None,))
    for share in ("1", "3", "5"):
        monkeypatch.setenv("FS_TRENDS_KSPLIT", share)
        again = check(index, monkeypatch, cols, n_works, unit_of, 17, when, q=4, P=33, seed=1,
                      products=(None,))
        for a, b in zip(first, again):
            assert a.tobytes() == b.tobytes()
    monkeypatch.delenv("FS_TRENDS_KSPLIT")
    ms = (C.c_double * 5)()
    assert _lib.load().fs_trends_times(ms) == abi.FS_OK
    assert ms[1] > 0 and ms[2] > 0 and abs(ms[4] - sum(ms[:4])) < 1e-9


# ---- family and degenerate units ---------------------------------------------------------

def test_family_ties_and_degenerate_units(index, monkeypatch):
    # units 0 and 3: the same works (bit 0 of a); unit 1: nobody; unit 2: every active work;
    # units 4 and 5: different works, as many
    def rule(a, u):
        return [a & 1, 0, 1, a & 1, a & 2, a & 4][u] != 0
    cols, n_works, unit_of, inc = case(64, 6, seed=3, rule=rule)
    act = active_numbers(cols)
    when = np.full(n_works, OUT, dtype=np.uint16)          # the pool: the active works alone
    when[act] = (act * 7) % 5
    units, perms, _ = check(index, monkeypatch, cols, n_works, unit_of, 6, when, q=1, P=33, seed=2)
    assert units["quoting"].tolist() == [32, 0, 64, 32, 32, 32]
    assert tuple(units[1]) == (0, 33, NONE, NONE, NONE, 0, 0, 0, 0)     # nobody quotes it
    assert tuple(units[2])[:3] == (64, 33, NONE) and units[2]["d"] == 0  # t = N: outside
    assert tuple(units[0]) == tuple(units[3])
    assert 3 not in perms["max_unit"].tolist() and 0 in perms["max_unit"].tolist()
    # min_quoting exactly at t(u) and one above it
    units, _, _ = check(index, monkeypatch, cols, n_works, unit_of, 6, when, q=32, P=33, seed=2)
    assert (units["adj_ge"] != NONE).tolist() == [True, False, False, True, True, True]
    units, perms, _ = check(index, monkeypatch, cols, n_works, unit_of, 6, when, q=33, P=33,
                            seed=2)
    assert (units["adj_ge"] == NONE).all() and (perms["max_unit"] == NONE).all()
    assert not perms["max_statistic"].any() and perms["offset_sum"].all()


def test_no_pool_work_active_no_records_no_units_and_an_empty_pool(index, monkeypatch):
    cols, n_works, unit_of, _ = case(10, 5, seed=2)
    act = active_numbers(cols)
    when = dates(n_works, seed=1, out=False)
    when[act] = OUT                                        # every active work outside the pool
    units, perms, sums = check(index, monkeypatch, cols, n_works, unit_of, 5, when, P=16)
    assert not sums.any() and (units["ge"] == 16).all() and (units["adj_ge"] == NONE).all()
    assert perms["offset_sum"].any() and (perms["max_unit"] == NONE).all()
    when = dates(n_works, seed=1)
    empty = (np.zeros(0, np.uint32),) * 3
    units, perms, sums = check(index, monkeypatch, empty, n_works, unit_of, 5, when, P=16)
    assert (units["ge"] == 16).all() and not sums.any() and perms["offset_sum"].any()
    units, perms, sums = check(index, monkeypatch, cols, n_works,
                               np.full(N_SCRIPT, NONE, np.uint32), 0, when, P=16)
    assert len(units) == 0 and sums.shape == (0, 16) and perms["offset_sum"].any()
    check(index, monkeypatch, cols, n_works, unit_of, 5, when, m=4, P=16)          # no passage
    units, perms, _ = check(index, monkeypatch, cols, n_works, unit_of, 5,
                            np.full(n_works, OUT, np.uint16), P=16)               # an empty pool
    assert not perms["offset_sum"].any() and (units["ge"] == 16).all()


# ---- 64-bit arithmetic and the bound -----------------------------------------------------

def test_a_million_pool_works_of_which_65_are_active(index, monkeypatch):
    """n_works at the bound: |D| << 10 needs more than 32 bits many times over, X_r is a sum
    over 2^20 works, and the gather reads a table of 2^20 offsets."""
    n_works = 1 << 20
    cols, small, unit_of, inc = case(65, 5, seed=12)
    act = active_numbers(cols)
    assert len(act) == 65
    spread = np.arange(small, dtype=np.int64) * ((n_works - 1) // (small - 1))
    spread[-1] = n_works - 1
    cols = (spread[cols[0]].astype(np.uint32), cols[1], cols[2])
    when = (np.arange(n_works, dtype=np.int64) * 2654435761 >> 7 & 1023).astype(np.uint16)
    when[spread[act[::2]]] = 1023
    units, perms, _ = check(index, monkeypatch, cols, n_works, unit_of, 5, when, q=2, P=2, seed=3,
                            device=False, fast=True, products=(None,))
    assert int(np.abs(units["d"]).max()) << 10 > 1 << 40
    assert (perms["offset_sum"] > 1 << 28).all() and (units["statistic"] > 1 << 10).any()


# ---- cross-checks ---------------------------------------------------------------------------

def test_two_seeds_differ_and_one_seed_repeats(index, monkeypatch):
    cols, n_works, unit_of, _ = case(65, 17, seed=9)
    when = dates(n_works, seed=6)
    one = check(index, monkeypatch, cols, n_works, unit_of, 17, when, P=33, seed=1)
    same = check(index, monkeypatch, cols, n_works, unit_of, 17, when, P=33, seed=1)
    other = check(index, monkeypatch, cols, n_works, unit_of, 17, when, P=33, seed=2)
    for a, b in zip(one, same):
        assert a.tobytes() == b.tobytes()
    assert (one[2] != other[2]).any() and one[0]["d"].tolist() == other[0]["d"].tolist()


# ---- refusals -----------------------------------------------------------------------------

def test_refusals_and_the_size_cap(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    import torch
    cols, n_works, unit_of, _ = case(65, 17, seed=9)
    good = dates(n_works, seed=6)

    def refused(c=cols, n_works=n_works, unit_of=unit_of, n_units=17, when=good, m=WIDTH, q=1,
                P=17, code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            trends.find_trends(*c, n_works, N_SCRIPT, unit_of, n_units, when[:n_works], m, 0, q,
                               P, 0)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        d_when = torch.from_numpy(np.ascontiguousarray(when).view(np.int16)).to("cuda")
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.trends_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(), n_units,
                                d_when.data_ptr(), m, 0, q, P, 0)
        assert e.value.code == code
        return str(e.value)
    refused(m=0)
    refused(q=0)
    refused(P=0)
    refused(P=4097)
    late = good.copy()
    late[n_works - 1] = 1024
    assert "`when` above 1023" in refused(when=late)
    refused(n_works=int(cols[0].max()))                    # a work >= n_works
    # and without a unit the records are checked all the same: one work, eight records, the last
    # of a work >= n_works
    stray = (np.array([0] * 7 + [1], np.uint32), np.arange(8, dtype=np.uint32),
             np.arange(10, 18, dtype=np.uint32))
    text = refused(stray, n_works=1, unit_of=np.full(N_SCRIPT, NONE, np.uint32), n_units=0,
                   when=np.zeros(1, np.uint16), m=3)
    assert "a work >= n_works or an orig_ix >= n_script" in text
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # an orig_ix >= n_script
    bad = unit_of.copy()
    bad[N_SCRIPT - 1] = 17                                 # neither below n_units nor none
    refused(unit_of=bad)
    # n_works above the bound: refused before a byte of `when` is read
    with pytest.raises(_lib.FsError) as e:
        trends.find_trends(*cols, (1 << 20) + 1, N_SCRIPT, unit_of, 17,
                           np.zeros((1 << 20) + 1, np.uint16), WIDTH, 0, 1, 17, 0)
    assert e.value.code == abi.FS_E_UNSUPPORTED
    # 65 active works, 18 rows padded to 32: a matrix of 64 x 2 x 8 bytes, two planes of
    # 32 x 128 bytes, 64 x 32 sums
    monkeypatch.setenv("FS_TRENDS_MAX_BYTES", str(1024 + 8192 + 8192 - 1))
    text = refused(code=abi.FS_E_UNSUPPORTED)
    assert "an incidence matrix of 1024 bytes" in text
    assert "two offset planes of 8192 bytes" in text and "sums of 8192 bytes" in text
    assert "more than 17407 bytes" in text
    monkeypatch.setenv("FS_TRENDS_MAX_BYTES", str(1024 + 8192 + 8192))
    check(index, monkeypatch, cols, n_works, unit_of, 17, good)        # at the bound: accepted
    monkeypatch.delenv("FS_TRENDS_MAX_BYTES")


# ---- the command ------------------------------------------------------------------------

def command(src, meta, by, unit, m, g, k, q, P, seed, more=()):
    argv = ["trends", src, meta, "--by", by, "--unit", unit, "--min-words", str(m),
            "--max-gap", str(g), "--min-works", str(k), "--min-quoting", str(q),
            "--permutations", str(P), "--seed", str(seed)]
    return main(argv + list(more))


@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case_,by,unit,m,g,k,q,P,seed", mtg.CASES)
def test_command_on_the_golden_input(tmp_path, case_, by, unit, m, g, k, q, P, seed, reader):
    src, meta = os.path.join(GOLDEN, mtg.INPUT), os.path.join(GOLDEN, mtg.META)
    prefix = str(tmp_path / "p")
    assert command(src, meta, by, unit, m, g, k, q, P, seed,
                   ["-o", prefix, "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in trends.output_names(src, prefix))
    for name, part in zip(mtg.golden_names(case_), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_the_default_prefix_and_a_file_without_records(tmp_path):
    import shutil
    src, meta = str(tmp_path / "m.csv"), os.path.join(GOLDEN, mtg.META)
    shutil.copy(os.path.join(GOLDEN, mtg.INPUT), src)
    assert main(["trends", src, meta, "--by", "month", "--unit", "character", "--permutations",
                 "20", "--seed", "3", "--min-quoting", "2"]) == 0
    with open(src, newline="", encoding="utf-8") as fh, \
            open(meta, newline="", encoding="utf-8") as mh:
        want = tr.trends_csv(fh.read(), mh.read(), "month", "character", min_quoting=2,
                             permutations=20, seed=3)
    for path, text in zip(trends.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[1].count("\r\n") == 1 + 47 + 2             # 2014-01 .. 2017-11, the last two
    assert want[2].count("\r\n") == 21
    with open(src, "w", newline="", encoding="utf-8") as fh:
        fh.write(open(os.path.join(GOLDEN, mtg.INPUT), newline="").readline())
    for reader in ("device", "python"):
        assert main(["trends", src, meta, "--reader", reader]) == 0
        for path, head in zip(trends.output_names(src),
                              (tr.UNIT_FIELDS, tr.PERIOD_FIELDS, tr.PERMUTATION_FIELDS)):
            with open(path, "rb") as fh:
                assert fh.read() == (",".join(head) + "\r\n").encode("utf-8")
