"""`companions` on the GPU: fs_companions and fs_companions_rows against the restated contract
(tests/companions_restated.py), every field of every unit and pair compared for equality;
numbers of units, of active works and lengths of runs around every size the kernels treat
differently; the regions of fs_quotes as units; `ao3.py companions` byte for byte against the
committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, companions, quotes, synth
from fandom_search_amd.cli import main
from tests import companions_restated as cr
from tests.golden import make_companions_golden as mcg
from tests.test_gpu_pairs import from_spans, interleaved, records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
# fs_tiles.h: units per tile of the incidence matrix, column tiles per workgroup, 64-bit words
# of active works per K-slice in LDS
TILE = 64
CHUNK = 8
K_SLICE = 32
N_SCRIPT = 3000          # of the index behind fs_companions_rows; every case uses it


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, m, g, b, s):
    recs = list(zip(*(c.tolist() for c in cols)))
    units, found = cr.companions(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units,
                                 m, g, b, s)
    u = np.zeros(n_units, dtype=abi.COMPANION_UNIT_DTYPE)
    for name in cr.UNIT_KEYS:
        u[name] = [d[name] for d in units]
    p = np.zeros(len(found), dtype=abi.COMPANION_DTYPE)
    for name in cr.PAIR_KEYS:
        p[name] = [d[name] for d in found]
    return u, p


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.COMPANION_UNIT_DTYPE, abi.COMPANION_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def on_device(cols, unit_of):
    """(rows tensor, unit map tensor) in HBM."""
    import torch
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name][:len(col)] = col
    return (torch.from_numpy(rows.view(np.uint8)).to("cuda"),
            torch.from_numpy(np.ascontiguousarray(unit_of, dtype=np.uint32)).to("cuda"))


def check(index, cols, n_works, unit_of, n_units, m=6, g=0, b=2, s=0):
    """Both entry points against the oracle; the host entry point's result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, n_works, unit_of, n_units, m, g, b, s)
    got = companions.find_companions(*cols, n_works, N_SCRIPT, unit_of, n_units, m, g, b, s)
    assert_equal(got, want)
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    dev = index.companions_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                  n_units, m, g, b, s)
    assert_equal(dev, want)
    return got


def blocks(n_units, seed, holes=0.05):
    """A unit map of n_units blocks of equal width over the script's front, the words behind
    them and a few inside them without a unit."""
    rng = np.random.default_rng(seed)
    width = max(1, (N_SCRIPT - 200) // n_units)
    o = np.arange(N_SCRIPT)
    unit_of = np.where(o // width < n_units, o // width, NONE).astype(np.uint32)
    unit_of[rng.random(N_SCRIPT) < holes] = NONE
    return unit_of


def random_works(n_active, seed, lo=3, hi=40, most=3):
    spans_of = interleaved(n_active, lambda k, rng: [
        (int(rng.integers(0, N_SCRIPT - hi)), int(rng.integers(lo, hi + 1)))
        for _ in range(int(rng.integers(1, most + 1)))], seed=seed)
    return from_spans(spans_of), len(spans_of)


# ---- sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_units", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                                     CHUNK * TILE - 1, CHUNK * TILE, CHUNK * TILE + 1])
def test_units_around_a_tile_and_a_chunk(index, n_units):
    cols, n_works = random_works(70, seed=n_units, hi=60, most=4)
    unit_of = blocks(n_units, seed=n_units)
    units, found = check(index, cols, n_works, unit_of, n_units, m=3, b=1)
    if n_units > 1:
        assert len(found) > 0 and found["b"].max() > found["a"].max()
    assert units["works"].sum() > 0
    check(index, cols, n_works, unit_of, n_units, m=3, b=2, s=30)


@pytest.mark.parametrize("n_active", [1, 63, 64, 65, K_SLICE * 64 - 1, K_SLICE * 64,
                                      K_SLICE * 64 + 1])
def test_active_works_around_a_word_and_a_slice(index, n_active):
    cols, n_works = random_works(n_active, seed=n_active, lo=3, hi=12, most=2)
    assert n_works > n_active                              # active numbers are not work numbers
    unit_of = blocks(37, seed=n_active)
    # the last active work, the last bit of the last 64-bit word, quotes units 0 and 36
    last = int(cols[0].max())
    width = (N_SCRIPT - 200) // 37
    more = from_spans([[]] * last + [[(0, 3), (36 * width, 3)]])
    unit_of[[0, 1, 2, 36 * width, 36 * width + 1, 36 * width + 2]] = [0, 0, 0, 36, 36, 36]
    keep = cols[0] != last
    cols = tuple(np.concatenate([c[keep], x]) for c, x in zip(cols, more))
    units, found = check(index, cols, n_works, unit_of, 37, m=3, b=1)
    both = [p for p in found if (p["a"], p["b"]) == (0, 36)]
    assert len(both) == 1 and both[0]["last_work"] == last
    if n_active > 1:
        check(index, cols, n_works, unit_of, 37, m=3, g=1, b=2, s=20)


def test_run_spans_that_start_mid_unit_cross_many_units_or_lie_in_no_unit(index):
    # 200 units of 3 words, 300 words without a unit, 10 units of 100 words, then none
    o = np.arange(N_SCRIPT)
    unit_of = np.full(N_SCRIPT, NONE, dtype=np.uint32)
    unit_of[:600] = o[:600] // 3
    unit_of[900:1900] = 200 + (o[900:1900] - 900) // 100
    spans_of = []
    for length in (1, 63, 64, 65, 200):
        for start in (1, 580, 601, 850, 1899, 2000):
            spans_of += [[(start, length), (1234, 1)]] * 2   # two works each: both >= 2
    cols = from_spans(spans_of)
    units, found = check(index, cols, len(spans_of), unit_of, 210, m=1, b=2)
    assert len(found) > 100
    assert units["works"][(1234 - 900) // 100 + 200] == len(spans_of)
    # unit 0: the ten runs from word 1; unit 199: the runs of 63 and more from word 580
    assert units["works"][0] == 10 and units["works"][199] == 8
    for start in (601, 2000):                              # wholly in words of no unit
        alone = from_spans([[(start, 200)], [(start, 200)]])
        units, found = check(index, alone, 2, unit_of, 210, m=1, b=1)
        assert not units["works"].any() and len(found) == 0
    check(index, cols, len(spans_of), unit_of, 210, m=64, b=2)   # the runs of 64 and more


# ---- content ----------------------------------------------------------------------------

def test_a_unit_nobody_quotes_and_every_work_quoting_every_unit(index):
    n_units = 2 * TILE + 2
    unit_of = np.full(N_SCRIPT, NONE, dtype=np.uint32)
    unit_of[:n_units * 2] = np.arange(n_units * 2) // 2
    unit_of[2 * 77:2 * 77 + 2] = NONE                      # unit 77 has no word left
    spans_of = interleaved(5, lambda k, rng: [(0, n_units * 2)], seed=3)
    units, found = check(index, from_spans(spans_of), len(spans_of), unit_of, n_units, m=3, b=5)
    assert tuple(units[77]) == (0, 0, NONE, 0)
    assert len(found) == (n_units - 1) * (n_units - 2) // 2    # all pairs of the others
    assert (found["a"] < found["b"]).all() and (found["both"] == 5).all()
    assert len(set(zip(found["a"].tolist(), found["b"].tolist()))) == len(found)
    others = np.arange(n_units) != 77
    assert (units["partners"][others] == n_units - 2).all()
    assert units["best"][0] == 1 and (units["best"][others][1:] == 0).all()
    # min_both above every count keeps nothing; the units keep their works
    none, found = check(index, from_spans(spans_of), len(spans_of), unit_of, n_units, m=3, b=6)
    assert len(found) == 0 and (none["works"] == units["works"]).all()
    assert (none["best"] == NONE).all() and not none["partners"].any()


def test_min_share_sweep_over_one_input(index):
    cols, n_works = random_works(150, seed=12, hi=80, most=4)
    unit_of = blocks(90, seed=12)
    kept = [len(check(index, cols, n_works, unit_of, 90, m=3, b=2, s=s)[1])
            for s in (0, 25, 50, 100)]
    assert kept[0] > 100 and kept[0] > kept[1] > kept[2] >= kept[3]
    L = _lib.load()
    ms = (C.c_double * 4)()
    assert L.fs_companions_times(ms) == abi.FS_OK and ms[0] > 0 and ms[1] > 0


# ---- errors and edges -------------------------------------------------------------------

def _call(L, cols, n_works, unit_of, n_units, m, b, s, units, found, cap, n, n_rows=None,
          n_script=N_SCRIPT):
    return L.fs_companions(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                           abi.ptr(cols[2], C.c_uint32),
                           len(cols[0]) if n_rows is None else n_rows, n_works, n_script,
                           abi.ptr(unit_of, C.c_uint32), n_units, m, 0, b, s,
                           units.ctypes.data_as(C.c_void_p),
                           found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


def test_capacity_too_small_by_one_exact_and_zero(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols, n_works = random_works(100, seed=8, hi=60)
    cols = [np.ascontiguousarray(c) for c in cols]
    unit_of = blocks(50, seed=8)
    want = oracle(cols, n_works, unit_of, 50, 3, 0, 2, 0)
    k = len(want[1])
    assert k > 10
    L = _lib.load()
    units = np.zeros(50, dtype=abi.COMPANION_UNIT_DTYPE)
    found = np.zeros(k, dtype=abi.COMPANION_DTYPE)
    n = C.c_uint64(0)
    for cap in (k - 1, 0):
        units[:] = 0
        assert _call(L, cols, n_works, unit_of, 50, 3, 2, 0, units, found, cap, n) == \
            abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((units, want[1]), want)               # the units are complete
        assert not found["b"].any()                        # the pairs untouched
    assert _call(L, cols, n_works, unit_of, 50, 3, 2, 0, units, found, k, n) == abi.FS_OK
    assert n.value == k
    assert_equal((units, found), want)
    # the caller's own device buffers
    d_rows, d_map = on_device(cols, unit_of)
    d_units = torch.zeros(50 * 16, dtype=torch.uint8, device="cuda")
    d_pairs = torch.zeros(k * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_units.data_ptr(), d_pairs.data_ptr())
    args = (d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(), 50, 3, 0, 2, 0)
    with pytest.raises(_lib.FsError) as e:
        index.companions_device(*args, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_units.cpu().numpy().view(abi.COMPANION_UNIT_DTYPE) == want[0]).all()
    assert not d_pairs.cpu().numpy().any()
    assert index.companions_device(*args, out_ptrs=ptrs, cap=k) == k
    assert (d_pairs.cpu().numpy().view(abi.COMPANION_DTYPE) == want[1]).all()
    # no records, and no units, on the device
    assert index.companions_device(d_rows.data_ptr(), 0, n_works, d_map.data_ptr(), 50, 3, 0, 2,
                                   0, out_ptrs=ptrs, cap=k) == 0
    none = d_units.cpu().numpy().view(abi.COMPANION_UNIT_DTYPE)
    assert (none["best"] == NONE).all() and not none["works"].any()
    assert index.companions_device(*args[:4], 0, 3, 0, 2, 0, out_ptrs=ptrs, cap=k) == 0


def test_no_records_and_no_units(index):
    empty = (np.zeros(0, np.uint32),) * 3
    unit_of = blocks(5, seed=1)
    units, found = check(index, empty, 3, unit_of, 5)
    assert units.tolist() == [(0, 0, NONE, 0)] * 5 and len(found) == 0
    cols, n_works = random_works(10, seed=2)
    units, found = check(index, cols, n_works, np.full(N_SCRIPT, NONE, np.uint32), 0, m=3)
    assert len(units) == 0 and len(found) == 0
    units, found = check(index, cols, n_works, unit_of, 5, m=41)     # no work has a passage
    assert units.tolist() == [(0, 0, NONE, 0)] * 5 and len(found) == 0
    # without a unit no record is read: one work, eight records, the last of a work >= n_works
    from fandom_search_amd.engine import torch_ready
    stray = (np.array([0] * 7 + [1], np.uint32), np.arange(8, dtype=np.uint32),
             np.arange(10, 18, dtype=np.uint32))
    no_unit = np.full(N_SCRIPT, NONE, np.uint32)
    d_rows, d_map = on_device(stray, no_unit)
    torch_ready()
    for units, found in (
            companions.find_companions(*stray, 1, N_SCRIPT, no_unit, 0, 3, 0, 2, 0),
            index.companions_device(d_rows.data_ptr(), 8, 1, d_map.data_ptr(), 0, 3, 0, 2, 0)):
        assert len(units) == 0 and len(found) == 0


def test_refusals(index):
    """include/fandom_search.h.  The accepted side of FS_COMPANIONS_MAX_BYTES, a matrix of 1 GiB,
    is not tested: only that one 64-bit word a row more is refused."""
    from fandom_search_amd.engine import torch_ready
    cols = records([300, 500, 200], N_SCRIPT, seed=9)
    unit_of = blocks(20, seed=9)

    def refused(c, n_works=3, unit_of=unit_of, n_units=20, m=6, b=2, s=0,
                code=abi.FS_E_INVALID, n_script=N_SCRIPT, rows=True):
        with pytest.raises(_lib.FsError) as e:
            companions.find_companions(*c, n_works, n_script, unit_of, n_units, m, 0, b, s)
        assert e.value.code == code
        if rows:
            d_rows, d_map = on_device(c, unit_of)
            torch_ready()
            with pytest.raises(_lib.FsError) as e:
                index.companions_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                        n_units, m, 0, b, s)
            assert e.value.code == code
    refused(cols, m=0)
    refused(cols, b=0)
    refused(cols, s=101)
    refused(cols, n_works=2)                               # a work >= n_works
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    bad = unit_of.copy()
    bad[N_SCRIPT - 1] = 20                                 # neither below n_units nor none
    refused(cols, unit_of=bad)
    bad[N_SCRIPT - 1] = NONE - 1
    refused(cols, unit_of=bad)
    big = np.full((1 << 19) + 1, NONE, dtype=np.uint32)
    refused(cols, unit_of=big, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED, rows=False)
    L = _lib.load()
    n = C.c_uint64(0)
    units = np.zeros(20, dtype=abi.COMPANION_UNIT_DTYPE)
    rc = _call(L, cols, 3, unit_of, 20, 6, 2, 0, units, units, 0, n, n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(index, cols, 3, unit_of, 20)                     # and the same columns are accepted
    # 16 385 works of one record each, a passage at --min-words 1: rows of 257 words of 8 bytes,
    # and 2^19 units of them are one word a row above FS_COMPANIONS_MAX_BYTES
    many = abi.FS_COMPANIONS_MAX_BYTES // (1 << 19) // 8 * 64 + 1
    assert many == 16385
    one = (np.arange(many, dtype=np.uint32), np.zeros(many, np.uint32),
           np.arange(many, dtype=np.uint32) % 2000)
    refused(one, n_works=many, n_units=1 << 19, m=1, b=1, code=abi.FS_E_UNSUPPORTED)
    units, found = companions.find_companions(*one, many, N_SCRIPT, unit_of, 20, 1, 0, 1, 0)
    assert units["works"].sum() >= 2000 * 0.9 * 8 and len(found) == 0   # a word a work: no pair


# ---- the regions of `quotes` as units ---------------------------------------------------

@pytest.mark.parametrize("g,k", [(0, 1), (2, 1), (0, 2)])
def test_works_of_a_region_are_the_n_works_of_quotes(index, g, k):
    # works of up to 60 records: sparse enough that --max-gap 2 does not merge the regions into
    # a handful (the oracle finds 112, 49 and 139 of them in the three cases)
    sizes = np.random.default_rng(20 + g).integers(0, 60, size=200)
    cols = records(sizes, N_SCRIPT, seed=20 + g)
    comb = np.zeros(len(cols[0]))
    words, regions = quotes.find_quotes(*cols, comb, 200, N_SCRIPT, 4, g, k)
    recs = list(zip(*(c.tolist() for c in cols)))
    _, bounds = cr.regions_of(cr.coverage(recs, 200, 4, g), N_SCRIPT, k)
    assert list(zip(regions["first"].tolist(), regions["last"].tolist())) == bounds
    assert len(regions) > 20
    unit_of = np.ascontiguousarray(words["region"])
    units, found = check(index, cols, 200, unit_of, len(regions), m=4, g=g, b=2)
    assert (units["works"] == regions["n_works"]).all() and len(found) > 0
    assert (units["works"] >= regions["peak"]).all()       # (its deepest word has no more)


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,by,m,g,k,b,s", mcg.CASES)
def test_command_on_the_golden_input(tmp_path, case, by, m, g, k, b, s, reader):
    src = os.path.join(GOLDEN, mcg.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["companions", src, "-o", prefix, "--by", by, "--min-words", str(m),
                 "--max-gap", str(g), "--min-works", str(k), "--min-both", str(b),
                 "--min-share", str(s), "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in companions.output_names(src, prefix))
    with open(src, newline="", encoding="utf-8") as fh:
        want = cr.companions_csv(fh.read(), by, m, g, k, b, s)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mcg.golden_names(case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_by_character_and_the_default_prefix(tmp_path):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, mcg.INPUT), src)
    assert main(["companions", src, "--by", "character", "--min-works", "7"]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        want = cr.companions_csv(fh.read(), "character")
    for path, text in zip(companions.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[0].count("\r\n") > 1
