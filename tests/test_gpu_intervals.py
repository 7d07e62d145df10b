"""`intervals` on the GPU: fs_intervals and fs_intervals_rows against the restated contract
(tests/intervals_restated.py), every field of both records compared for equality, with the
product by MFMA (FS_INTERVALS_MFMA unset) and by the plain kernel (0); active works, units and
replicates around every size the kernels treat differently; an incidence that no swap of row and
column in a fragment map leaves unchanged; `ao3.py intervals` byte for byte against the committed
files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, companions, intervals, synth
from fandom_search_amd.cli import main
from tests import intervals_restated as ir
from tests.golden import make_intervals_golden as mig
from tests.test_gpu_companions import on_device
from tests.test_gpu_pairs import from_spans, interleaved

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
N_SCRIPT = 3000          # of the index behind fs_intervals_rows; every case uses it
WIDTH = 3                # script words of a unit in the synthetic cases, and their --min-words


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, m, g, B, seed, level, fast=False):
    recs = list(zip(*(c.tolist() for c in cols)))
    units, reps = ir.intervals(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units, m,
                               g, B, seed, level, fast=fast)
    u = np.zeros(n_units, dtype=abi.INTERVAL_UNIT_DTYPE)
    for name in ir.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    r = np.zeros(B, dtype=abi.INTERVAL_REPLICATE_DTYPE)
    for name in ir.REPLICATE_KEYS:
        r[name] = [d[name] for d in reps]
    return u, r


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.INTERVAL_UNIT_DTYPE, abi.INTERVAL_REPLICATE_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def check(index, monkeypatch, cols, n_works, unit_of, n_units, m=WIDTH, g=0, B=17, seed=0,
          level=95, fast=False):
    """Both entry points under both products against the oracle; the host entry point's
    result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, n_works, unit_of, n_units, m, g, B, seed, level, fast)
    d_rows, d_map = on_device(cols, unit_of)
    for mfma in (None, "0"):
        if mfma is None:
            monkeypatch.delenv("FS_INTERVALS_MFMA", raising=False)
        else:
            monkeypatch.setenv("FS_INTERVALS_MFMA", mfma)
        got = intervals.find_intervals(*cols, n_works, N_SCRIPT, unit_of, n_units, m, g, B, seed,
                                       level)
        assert_equal(got, want)
        torch_ready()
        dev = index.intervals_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                     n_units, m, g, B, seed, level)
        assert_equal(dev, want)
    monkeypatch.delenv("FS_INTERVALS_MFMA", raising=False)
    return got


def quoted(a, u):
    """The asymmetric incidence: active work a quotes unit u when bit u % 7 of a, XORed with a
    constant of the unit, is set."""
    return ((a ^ (u * 37 + 11)) >> (u % 7)) & 1 == 1


def mixed(a, u):
    """An incidence without the few distinct rows of quoted(): a bit of a product of both."""
    return (((a + 1) * (2 * u + 3) * 2654435761) >> 13) & 1 == 1


def case(n_active, n_units, seed, rule=quoted):
    """(cols, n_works, unit_of, inc): unit u owns the script words 3 u .. 3 u + 2; active work
    a quotes the units `rule` gives it, at least one (the last unit otherwise), each by a run of
    its own; works without a passage lie between the active ones.  inc[u][a] is the incidence
    over active numbers."""
    inc = np.zeros((n_units, n_active), dtype=np.int64)
    for a in range(n_active):
        mine = [u for u in range(n_units) if rule(a, u)] or [n_units - 1]
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
def test_active_works_around_a_k_step(index, monkeypatch, n_active):
    cols, n_works, unit_of, inc = case(n_active, 17, seed=n_active)
    assert n_works > n_active                              # active numbers are not work numbers
    units, reps = check(index, monkeypatch, cols, n_works, unit_of, 17, seed=n_active)
    assert (units["works"] == inc.sum(axis=1)).all()
    assert (reps["resampled_works"] >= reps["resampled_active"]).all()
    assert (reps["resampled_works"] != reps["resampled_active"]).any()    # inactive works drawn


@pytest.mark.parametrize("n_units", [1, 15, 16, 17, 64, 65])
def test_units_around_a_fragment_and_a_tile(index, monkeypatch, n_units):
    cols, n_works, unit_of, inc = case(65, n_units, seed=100 + n_units)
    units, _ = check(index, monkeypatch, cols, n_works, unit_of, n_units, seed=5)
    assert (units["works"] == inc.sum(axis=1)).all() and units["works"].sum() > 0
    assert (units["ahead"] + units["tied"] + units["behind"])[units["next"] != NONE].tolist() == \
        [17] * (n_units - 1)


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_replicates_around_a_fragment(index, monkeypatch, B):
    cols, n_works, unit_of, _ = case(65, 17, seed=200 + B)
    for level in (50, 95, 99):
        units, reps = check(index, monkeypatch, cols, n_works, unit_of, 17, B=B, seed=B,
                            level=level)
        assert (units["works_low"] <= units["works_median"]).all()
        assert (units["works_median"] <= units["works_high"]).all()
    assert len(reps) == B


def test_the_most_replicates_the_sort_in_lds_takes(index, monkeypatch):
    cols, n_works, unit_of, _ = case(20, 5, seed=7)
    units, reps = check(index, monkeypatch, cols, n_works, unit_of, 5, B=4096, seed=11,
                        fast=True)
    assert len(reps) == 4096 and (units["works_low"] < units["works_high"]).all()
    # B = 4095: a power of two less one, one padded entry above the sorted ones
    check(index, monkeypatch, cols, n_works, unit_of, 5, B=4095, seed=11, level=99, fast=True)


@pytest.mark.parametrize("n_active,ksplit", [(129, "2"), (129, "3"), (129, "9"), (1100, None)])
def test_the_words_of_a_tile_shared_among_workgroups(index, monkeypatch, n_active, ksplit):
    """Few tiles: the product's workgroups share the words k and add their parts.  Three words
    in two, three and (more shares than words) nine parts; 1100 works are 18 words, which one
    tile shares out by itself, three parts of at least 8 words."""
    if ksplit is not None:
        monkeypatch.setenv("FS_INTERVALS_KSPLIT", ksplit)
    cols, n_works, unit_of, inc = case(n_active, 17, seed=300 + n_active, rule=mixed)
    units, _ = check(index, monkeypatch, cols, n_works, unit_of, 17, B=33, seed=4)
    assert (units["works"] == inc.sum(axis=1)).all()


# ---- content ----------------------------------------------------------------------------

def test_incidence_alone_at_one_replicate(index, monkeypatch):
    """With one replicate LOW = MEDIAN = HIGH = c_0(u): the counts are mult @ incidence, and
    nothing else of the contract is looked at."""
    cols, n_works, unit_of, inc = case(129, 65, seed=31, rule=mixed)
    assert len({tuple(r) for r in inc.tolist()}) == 65 and (inc[:64, :64] != inc[:64, :64].T).any()
    act = active_numbers(cols)
    assert len(act) == 129
    for seed in (0, 9):
        want = inc @ ir.mult_np(seed, [0], act).astype(np.int64)[0]
        assert want.max() > 13 and len(set(want.tolist())) > 20
        for mfma in (None, "0"):
            if mfma is None:
                monkeypatch.delenv("FS_INTERVALS_MFMA", raising=False)
            else:
                monkeypatch.setenv("FS_INTERVALS_MFMA", mfma)
            units, reps = intervals.find_intervals(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0,
                                                   1, seed, 95)
            assert units["works_low"].tolist() == want.tolist(), mfma
            # RESAMPLED_WORKS is the host's sum over every work of the file
            assert int(reps["resampled_works"][0]) == \
                int(ir.mult_np(seed, [0], range(n_works)).sum())
            assert int(reps["resampled_active"][0]) == int(ir.mult_np(seed, [0], act).sum())


def test_a_swap_in_a_fragment_map_would_change_a_count():
    """What makes the asymmetric case a check of the maps: neither the incidence nor the
    multiplicities are symmetric, in rows, columns or their 16 x 16 blocks."""
    inc = np.array([[quoted(a, u) for a in range(64)] for u in range(64)], dtype=np.int64)
    m = ir.mult_np(0, range(64), range(64)).astype(np.int64)
    assert (inc != inc.T).any() and (m != m.T).any()
    right = inc @ m.T                                          # counts[u][b]
    assert (right != right.T).any()
    assert (right != inc.T @ m.T).any() and (right != inc @ m).any()
    for blk in (inc[:16, :16], m[:16, :16], right[:16, :16]):
        assert (blk != blk.T).any()


def test_a_unit_nobody_quotes_two_units_with_the_same_works_and_ties_around_next(
        index, monkeypatch):
    # units 0 and 3: the same works (bit 0 of a); unit 1: nobody; unit 2: every work; units 4
    # and 5: different works, as many (bits 1 and 2 over 64 works)
    def rule(a, u):
        return [a & 1, 0, 1, a & 1, a & 2, a & 4][u] != 0
    cols, n_works, unit_of, inc = case(64, 6, seed=3, rule=rule)
    units, reps = check(index, monkeypatch, cols, n_works, unit_of, 6, B=33, seed=2)
    assert units["works"].tolist() == [32, 0, 64, 32, 32, 32]
    assert units["rank"].tolist() == [2, 6, 1, 2, 2, 2]
    assert units["next"].tolist() == [3, NONE, 0, 4, 5, 1]         # 2, 0, 3, 4, 5, 1
    assert tuple(units[0][["ahead", "tied", "behind"]]) == (0, 33, 0)
    assert units["ahead"][3] > 0 and units["behind"][3] > 0       # as many works, other works
    one = units[1]
    assert [int(one[k]) for k in ir.UNIT_KEYS] == [0, 0, 0, 0, 0, 0, 0, 0, 6, NONE, 0, 0, 0, 0]
    assert units["behind"][5] == 0 and units["ahead"][5] + units["tied"][5] == 33
    assert reps["units_quoted"].max() == 5


def test_works_are_those_of_companions(index, monkeypatch):
    cols, n_works, unit_of, _ = case(129, 65, seed=41, rule=mixed)
    units, _ = check(index, monkeypatch, cols, n_works, unit_of, 65, B=16, seed=1)
    theirs, _ = companions.find_companions(*cols, n_works, N_SCRIPT, unit_of, 65, WIDTH, 0, 2, 0)
    assert (units["works"] == theirs["works"]).all() and (units["works"] > 0).sum() >= 64
    L = _lib.load()
    ms = (C.c_double * 6)()
    assert L.fs_intervals_times(ms) == abi.FS_OK
    assert ms[2] > 0 and abs(ms[5] - sum(ms[:5])) < 1e-9


# ---- errors and edges -------------------------------------------------------------------

def test_no_records_no_units_and_no_active_work(index, monkeypatch):
    empty = (np.zeros(0, np.uint32),) * 3
    cols, n_works, unit_of, _ = case(10, 5, seed=2)
    units, reps = check(index, monkeypatch, empty, 3, unit_of, 5, B=16)
    assert units["next"].tolist() == [1, 2, 3, 4, NONE] and units["tied"].tolist() == [16] * 4 + [0]
    assert not units["works"].any() and (units["rank"] == 1).all()
    assert not reps["resampled_active"].any() and reps["resampled_works"].sum() > 0
    units, reps = check(index, monkeypatch, cols, n_works, np.full(N_SCRIPT, NONE, np.uint32), 0)
    assert len(units) == 0 and reps["resampled_active"].sum() > 0
    units, reps = check(index, monkeypatch, cols, n_works, unit_of, 5, m=4)   # no passage
    assert not units["works"].any() and not reps["resampled_active"].any()


def test_refusals_and_the_size_cap(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    cols, n_works, unit_of, _ = case(65, 17, seed=9)

    def refused(c=cols, n_works=n_works, unit_of=unit_of, n_units=17, m=WIDTH, B=17, level=95,
                code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            intervals.find_intervals(*c, n_works, N_SCRIPT, unit_of, n_units, m, 0, B, 0, level)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.intervals_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                   n_units, m, 0, B, 0, level)
        assert e.value.code == code
        return str(e.value)
    refused(m=0)
    refused(B=0)
    refused(B=4097)
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
    refused(unit_of=bad)
    # 65 active works: a matrix of 64 x 2 x 8 bytes, 32 x 128 multiplicity bytes, 64 x 32 counts
    monkeypatch.setenv("FS_INTERVALS_MAX_BYTES", str(1024 + 4096 + 8192 - 1))
    text = refused(code=abi.FS_E_UNSUPPORTED)
    assert "an incidence matrix of 1024 bytes" in text
    assert "multiplicities of 4096 bytes" in text and "counts of 8192 bytes" in text
    assert "more than 13311 bytes" in text
    monkeypatch.setenv("FS_INTERVALS_MAX_BYTES", str(1024 + 4096 + 8192))
    check(index, monkeypatch, cols, n_works, unit_of, 17)  # at the bound: accepted
    monkeypatch.delenv("FS_INTERVALS_MAX_BYTES")


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case_,by,m,g,k,B,seed,level", mig.CASES)
def test_command_on_the_golden_input(tmp_path, case_, by, m, g, k, B, seed, level, reader):
    src = os.path.join(GOLDEN, mig.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["intervals", src, "-o", prefix, "--by", by, "--min-words", str(m),
                 "--max-gap", str(g), "--min-works", str(k), "--replicates", str(B),
                 "--seed", str(seed), "--level", str(level), "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in intervals.output_names(src, prefix))
    for name, part in zip(mig.golden_names(case_), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_by_character_the_default_prefix_and_a_file_without_records(tmp_path):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, mig.INPUT), src)
    assert main(["intervals", src, "--by", "character", "--replicates", "20", "--seed", "3"]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        want = ir.intervals_csv(fh.read(), "character", replicates=20, seed=3)
    for path, text in zip(intervals.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[0].count("\r\n") == 5 and want[1].count("\r\n") == 21
    with open(src, "w", newline="", encoding="utf-8") as fh:
        fh.write(open(os.path.join(GOLDEN, mig.INPUT), newline="").readline())
    for reader in ("device", "python"):
        assert main(["intervals", src, "--reader", reader]) == 0
        for path, head in zip(intervals.output_names(src),
                              (ir.UNIT_FIELDS, ir.REPLICATE_FIELDS)):
            with open(path, "rb") as fh:
                assert fh.read() == (",".join(head) + "\r\n").encode("utf-8")
