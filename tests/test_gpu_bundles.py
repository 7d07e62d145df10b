"""`bundles` on the GPU: fs_bundles and fs_bundles_rows against the restated contract
(tests/bundles_restated.py), every field of every unit, level and set compared for equality,
the reserved words too, with FS_BUNDLES_PRUNE on and off; numbers of units, of active works and
of a parent's extensions around every size the kernels treat differently; the cap on a level,
the growing buffer, level 2 against fs_companions; `ao3.py bundles` byte for byte against the
committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, bundles, companions, synth
from fandom_search_amd.cli import main
from tests import bundles_restated as br
from tests.golden import make_bundles_golden as mbg
from tests.test_bundles_host import as_records
from tests.test_gpu_companions import on_device
from tests.test_gpu_pairs import from_spans, interleaved

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
# fs_tiles.h: units per tile of the incidence matrix, column tiles per workgroup, 64-bit words
# of active works per K-slice of the level-2 tiles; fs_bundles.hip: words per K-slice of the
# count pass, extensions of a parent per work item
TILE = 64
CHUNK = 8
K_SLICE = 32
COUNT_SLICE = 256
PIECE = 64
N_SCRIPT = 3000          # of the index behind fs_bundles_rows; every case uses it
WIDTH = 3                # script words of a unit in the cases made by quoting()
DTYPES = (abi.BUNDLE_UNIT_DTYPE, abi.BUNDLE_LEVEL_DTYPE, abi.BUNDLE_DTYPE)


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, unit_of, n_units, m, g, a, k):
    recs = list(zip(*(c.tolist() for c in cols)))
    return as_records(*br.bundles(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units,
                                  m, g, a, k))


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names if len(a) else ():            # (the reserved words, 0, too)
            bad = np.nonzero((a[name] != b[name]).reshape(len(a), -1).any(axis=1))[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


class environment(object):
    """A switch of the library's, read on each call, set for the calls inside."""

    def __init__(self, name, value):
        self.name, self.value = name, str(value)

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def check(index, cols, n_works, unit_of, n_units, m=3, g=0, a=2, k=4):
    """Both entry points, and the host one without pruning, against the oracle; the host entry
    point's result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, n_works, unit_of, n_units, m, g, a, k)
    got = bundles.find_bundles(*cols, n_works, N_SCRIPT, unit_of, n_units, m, g, a, k)
    assert_equal(got, want)
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    dev = index.bundles_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                               n_units, m, g, a, k)
    assert_equal(dev, want)
    with environment("FS_BUNDLES_PRUNE", 0):
        plain = bundles.find_bundles(*cols, n_works, N_SCRIPT, unit_of, n_units, m, g, a, k)
    assert_equal(plain, want)
    return got


def unit_map(n_units):
    """Unit u is the script words WIDTH u .. WIDTH u + WIDTH - 1; the words behind have none."""
    o = np.arange(N_SCRIPT)
    assert n_units * WIDTH <= N_SCRIPT
    return np.where(o // WIDTH < n_units, o // WIDTH, NONE).astype(np.uint32)


def quoting(units_of_work, seed=0):
    """(columns, n_works) of active works that each quote the units listed for them, a passage
    of WIDTH words per unit, with works without a passage in between."""
    spans_of = interleaved(len(units_of_work), lambda k, rng: [
        (int(u) * WIDTH, WIDTH) for u in units_of_work[k]], seed=seed)
    return from_spans(spans_of), len(spans_of)


def hot_and_cold(n_units, n_active, seed, hot=6, take=3, cold=2):
    """Every work quotes `take` of the `hot` units, which are spread over all tiles, and `cold`
    others: sets of the hot ones are frequent, across the tile and chunk boundaries."""
    rng = np.random.default_rng(seed)
    hot_units = np.unique(np.linspace(0, n_units - 1, min(hot, n_units)).astype(int))
    out = []
    for _ in range(n_active):
        mine = set(rng.choice(hot_units, size=min(take, len(hot_units)), replace=False).tolist())
        mine |= set(rng.integers(0, n_units, size=cold).tolist())
        out.append(sorted(mine))
    return out


# ---- sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_units", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1,
                                     CHUNK * TILE - 1, CHUNK * TILE + 1])
def test_units_around_a_tile_and_a_chunk(index, n_units):
    cols, n_works = quoting(hot_and_cold(n_units, 70, seed=n_units), seed=n_units)
    units, levels, sets = check(index, cols, n_works, unit_map(n_units), n_units, a=2, k=3)
    assert units["works"].sum() > 0 and list(levels["size"]) == [2, 3, 4]
    if n_units > 2:
        assert len(sets) > 0 and (sets["size"] == 3).any()
        assert sets["units"][:, 1].max() == n_units - 1    # the last unit of the last tile
    else:
        assert (levels["frequent"][1:] == 0).all()


@pytest.mark.parametrize("n_active", [1, 63, 64, 65, K_SLICE * 64 - 1, K_SLICE * 64,
                                      K_SLICE * 64 + 1, COUNT_SLICE * 64, COUNT_SLICE * 64 + 1])
def test_active_works_around_a_word_and_a_slice(index, n_active):
    rng = np.random.default_rng(n_active)
    of_work = [sorted(rng.choice(12, size=3, replace=False).tolist())
               for _ in range(n_active - 1)]
    of_work.append([0, 5, 11])         # the last active work, the last bit of the last word
    cols, n_works = quoting(of_work, seed=n_active)
    assert n_works > n_active                              # active numbers are not work numbers
    bar = max(1, n_active // 300)
    units, levels, sets = check(index, cols, n_works, unit_map(12), 12, a=bar, k=3)
    assert units["works"].sum() == 3 * n_active
    assert levels["frequent"][1] > 0 or n_active < 3
    last = sets[(sets["units"][:, :3] == [0, 5, 11]).all(axis=1)]
    assert len(last) == 1 and last[0]["works"] >= 1
    if n_active == 1:
        assert last[0]["first_work"] == int(cols[0].max()) and last[0]["closed"] == 1


@pytest.mark.parametrize("group", [1, 2, PIECE - 1, PIECE, PIECE + 1, 300])
def test_a_parent_with_so_many_extensions(index, group):
    """Units 0 and 1 with one of the units 2 .. group + 1, two works each: the parent (0, 1)
    has `group` extensions, all frequent, (0, x) has the (0, y) behind it, none frequent and
    every one pruned; 300 extensions are five work items."""
    of_work = [[0, 1, x] for x in range(2, group + 2) for _ in range(2)]
    cols, n_works = quoting(of_work, seed=group)
    n_units = group + 3                                    # and a unit nobody quotes
    units, levels, sets = check(index, cols, n_works, unit_map(n_units), n_units, a=2, k=3)
    assert levels["frequent"].tolist() == [2 * group + 1, group, 0]
    assert levels["candidates"][1] == group + group * (group - 1)
    assert levels["candidates"][2] == group * (group - 1) // 2
    three = sets[sets["size"] == 3]
    assert (three["units"][:, 2] == np.arange(2, group + 2)).all()
    assert (three["works"] == 2).all() and (three["closed"] == 1).all()
    assert tuple(units[n_units - 1]) == (0, 0, 0, 0)
    assert tuple(units[0]) == (2 * group, group + 1 + group, 3, 0)   # its pairs, its triples


# ---- content ----------------------------------------------------------------------------

def test_a_clique_of_nine_units_under_max_size_eight_and_three(index):
    of_work = [list(range(2, 11))] * 5 + [[0, 2], [12]]
    cols, n_works = quoting(of_work, seed=9)
    units, levels, sets = check(index, cols, n_works, unit_map(14), 14, a=5, k=8)
    assert [int((sets["size"] == s).sum()) for s in range(2, 9)] == [36, 84, 126, 126, 84, 36, 9]
    assert levels["frequent"].tolist() == [36, 84, 126, 126, 84, 36, 9, 1]   # the 9-set: mined
    assert not sets["closed"].any()                        # not even a set of eight
    assert (sets["extensions"] == 9 - sets["size"]).all()
    assert levels["closed"].tolist() == [0] * 7 + [NONE]
    assert tuple(units[1]) == (0, 0, 0, 0) and tuple(units[13]) == (0, 0, 0, 0)
    assert tuple(units[0]) == (1, 0, 0, 0) and units["largest"][2:11].tolist() == [8] * 9
    units, levels, sets = check(index, cols, n_works, unit_map(14), 14, a=5, k=3)
    assert levels["frequent"].tolist() == [36, 84, 126] and len(sets) == 120
    assert (sets["extensions"][sets["size"] == 3] == 6).all()
    # a sixth work quoting eight of the nine: that set of eight is closed, the others are not
    cols, n_works = quoting(of_work + [list(range(2, 10))], seed=9)
    units, levels, sets = check(index, cols, n_works, unit_map(14), 14, a=5, k=8)
    eight = sets[sets["size"] == 8]
    assert eight["closed"].tolist() == [1] + [0] * 8 and eight["works"].tolist() == [6] + [5] * 8


def test_identical_works_and_the_bar_at_and_above_them(index):
    of_work = [[0, 1, 2, 3, 4]] * 129
    cols, n_works = quoting(of_work, seed=5)
    units, levels, sets = check(index, cols, n_works, unit_map(5), 5, a=129, k=4)
    assert levels["frequent"].tolist() == [10, 10, 5, 1] and (sets["works"] == 129).all()
    assert (sets["first_work"] == int(cols[0].min())).all()
    units, levels, sets = check(index, cols, n_works, unit_map(5), 5, a=130, k=4)
    assert len(sets) == 0 and not levels["candidates"].any()
    assert (units["works"] == 129).all() and not units["sets"].any()


def test_a_unit_exactly_at_the_bar_and_one_below(index):
    of_work = [[0, 1, 2]] * 3 + [[0, 1]] * 2 + [[0, 2]]    # works: 6, 5, 4
    cols, n_works = quoting(of_work, seed=6)
    units, levels, sets = check(index, cols, n_works, unit_map(3), 3, a=4, k=4)
    assert units["works"].tolist() == [6, 5, 4]
    assert [(s["units"][:2].tolist(), int(s["works"])) for s in sets] == \
        [([0, 1], 5), ([0, 2], 4)]
    assert levels["candidates"].tolist()[:2] == [3, 1] and levels["frequent"][1] == 0
    units, levels, sets = check(index, cols, n_works, unit_map(3), 3, a=5, k=4)
    assert levels["candidates"][0] == 1 and len(sets) == 1     # unit 2 is one work short
    units, levels, sets = check(index, cols, n_works, unit_map(3), 3, a=3, k=4)
    assert [int(s["closed"]) for s in sets] == [1, 1, 0, 1] and sets[3]["size"] == 3


def test_one_work_is_enough_at_min_all_one(index):
    cols, n_works = quoting(hot_and_cold(40, 25, seed=4, hot=8, take=4, cold=1), seed=4)
    units, levels, sets = check(index, cols, n_works, unit_map(40), 40, a=1, k=4)
    assert (sets["works"] == 1).any() and (sets["size"] == 4).any()
    assert levels["frequent"][3] > 0                       # sets of five: a work's whole list
    L = _lib.load()
    ms = (C.c_double * abi.FS_BUNDLES_TIMES)()
    assert L.fs_bundles_times(ms) == abi.FS_OK
    assert ms[0] > 0 and ms[1] > 0 and ms[3] > 0 and ms[31] >= ms[0] + ms[1] + ms[3]


# ---- the cap, the growing buffer, level 2 -----------------------------------------------

def _call(L, cols, n_works, unit_of, n_units, a, k, units, levels, found, cap, n):
    return L.fs_bundles(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                        abi.ptr(cols[2], C.c_uint32), len(cols[0]), n_works, N_SCRIPT,
                        abi.ptr(unit_of, C.c_uint32), n_units, WIDTH, 0, a, k,
                        units.ctypes.data_as(C.c_void_p), levels.ctypes.data_as(C.c_void_p),
                        found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


def test_a_level_one_above_the_cap_is_refused_and_one_at_it_is_not(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols, n_works = quoting([[0, 1, 2, 3, 4, 5]] * 2, seed=2)
    cols = [np.ascontiguousarray(c) for c in cols]
    unit_of = unit_map(6)
    want = oracle(cols, n_works, unit_of, 6, WIDTH, 0, 2, 4)
    assert want[1]["candidates"].tolist() == [15, 20, 15, 6]
    L = _lib.load()
    units = np.ones(6, dtype=abi.BUNDLE_UNIT_DTYPE)
    levels = np.ones(4, dtype=abi.BUNDLE_LEVEL_DTYPE)
    found = np.ones(50, dtype=abi.BUNDLE_DTYPE)
    before = [x.tobytes() for x in (units, levels, found)]
    n = C.c_uint64(0)
    d_rows, d_map = on_device(cols, unit_of)
    d_out = [torch.ones(len(x) * x.dtype.itemsize, dtype=torch.uint8, device="cuda")
             for x in (units, levels, found)]
    torch_ready()
    for cap, level, count in ((19, 3, 20), (14, 2, 15)):
        with environment("FS_BUNDLES_MAX_SETS", cap):
            assert _call(L, cols, n_works, unit_of, 6, 2, 4, units, levels, found, 50, n) == \
                abi.FS_E_UNSUPPORTED
            text = L.fs_last_error().decode()
            assert "level %d has %d candidate sets" % (level, count) in text
            assert "--min-all" in text and "--max-size" in text
            for x, was in zip((units, levels, found), before):   # the output buffers untouched
                assert x.tobytes() == was
            with pytest.raises(_lib.FsError) as e:
                index.bundles_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                     6, WIDTH, 0, 2, 4, out_ptrs=[t.data_ptr() for t in d_out],
                                     cap=50)
            assert e.value.code == abi.FS_E_UNSUPPORTED
            assert all(bool((t == 1).all()) for t in d_out)
    with environment("FS_BUNDLES_MAX_SETS", 20):
        assert _call(L, cols, n_works, unit_of, 6, 2, 4, units, levels, found, 50, n) == abi.FS_OK
    assert n.value == 50
    assert_equal((units, levels, found), want)


def test_capacity_grows_from_one(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols, n_works = quoting(hot_and_cold(30, 60, seed=8), seed=8)
    cols = [np.ascontiguousarray(c) for c in cols]
    unit_of = unit_map(30)
    want = oracle(cols, n_works, unit_of, 30, WIDTH, 0, 2, 4)
    k = len(want[2])
    assert k > 10
    L = _lib.load()
    units = np.zeros(30, dtype=abi.BUNDLE_UNIT_DTYPE)
    levels = np.zeros(4, dtype=abi.BUNDLE_LEVEL_DTYPE)
    found = np.zeros(k, dtype=abi.BUNDLE_DTYPE)
    n = C.c_uint64(0)
    for cap in (1, k - 1, 0):
        units[:] = 0
        levels[:] = 0
        assert _call(L, cols, n_works, unit_of, 30, 2, 4, units, levels, found, cap, n) == \
            abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((units, levels, want[2]), want)       # the units and levels are complete
        assert not found.view(np.uint8).any()              # the sets untouched
    assert _call(L, cols, n_works, unit_of, 30, 2, 4, units, levels, found, k, n) == abi.FS_OK
    assert_equal((units, levels, found), want)
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    args = (d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(), 30, WIDTH, 0, 2, 4)
    assert_equal(index.bundles_device(*args, cap=1), want)   # grown by the wrapper
    d_out = [torch.zeros(len(x) * x.dtype.itemsize, dtype=torch.uint8, device="cuda")
             for x in (units, levels, found)]
    torch_ready()
    ptrs = [t.data_ptr() for t in d_out]
    with pytest.raises(_lib.FsError) as e:
        index.bundles_device(*args, out_ptrs=ptrs, cap=1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_out[0].cpu().numpy().view(abi.BUNDLE_UNIT_DTYPE) == want[0]).all()
    assert (d_out[1].cpu().numpy().view(abi.BUNDLE_LEVEL_DTYPE) == want[1]).all()
    assert not d_out[2].cpu().numpy().any()
    assert index.bundles_device(*args, out_ptrs=ptrs, cap=k) == k
    assert (d_out[2].cpu().numpy().view(abi.BUNDLE_DTYPE) == want[2]).all()
    # no records, and no units, on the device
    assert index.bundles_device(d_rows.data_ptr(), 0, n_works, d_map.data_ptr(), 30, WIDTH, 0, 2,
                                4, out_ptrs=ptrs, cap=k) == 0
    assert not d_out[0].cpu().numpy().any()
    assert index.bundles_device(*args[:4], 0, WIDTH, 0, 2, 4, out_ptrs=ptrs, cap=k) == 0


def test_level_two_is_the_pairs_of_companions(index):
    cols, n_works = quoting(hot_and_cold(90, 150, seed=12, hot=10, take=4, cold=3), seed=12)
    unit_of = unit_map(90)
    for bar in (1, 2, 7):
        units, levels, sets = bundles.find_bundles(*cols, n_works, N_SCRIPT, unit_of, 90, WIDTH,
                                                   0, bar, 2)
        cu, pairs = companions.find_companions(*cols, n_works, N_SCRIPT, unit_of, 90, WIDTH, 0,
                                               bar, 0)
        two = sets[sets["size"] == 2]
        assert len(two) == len(pairs) == len(sets) > 0
        assert (two["units"][:, 0] == pairs["a"]).all() and (two["units"][:, 1] == pairs["b"]).all()
        assert (two["works"] == pairs["both"]).all()
        assert (two["first_work"] == pairs["first_work"]).all()
        assert (units["works"] == cu["works"]).all()
        assert (two["units"][:, 2:] == NONE).all()


def test_no_records_no_units_and_no_passage(index):
    empty = (np.zeros(0, np.uint32),) * 3
    units, levels, sets = check(index, empty, 3, unit_map(5), 5)
    assert units.tolist() == [(0, 0, 0, 0)] * 5 and len(sets) == 0
    assert levels.tolist() == [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0),
                               (5, 0, 0, NONE, NONE)]
    cols, n_works = quoting([[0, 1]] * 3, seed=1)
    units, levels, sets = check(index, cols, n_works, np.full(N_SCRIPT, NONE, np.uint32), 0)
    assert len(units) == 0 and len(sets) == 0
    units, levels, sets = check(index, cols, n_works, unit_map(5), 5, m=WIDTH + 1)
    assert units.tolist() == [(0, 0, 0, 0)] * 5 and len(sets) == 0
    # without a unit no record is read: one work, eight records, the last of a work >= n_works
    from fandom_search_amd.engine import torch_ready
    stray = (np.array([0] * 7 + [1], np.uint32), np.arange(8, dtype=np.uint32),
             np.arange(10, 18, dtype=np.uint32))
    no_unit = np.full(N_SCRIPT, NONE, np.uint32)
    d_rows, d_map = on_device(stray, no_unit)
    torch_ready()
    for units, levels, sets in (
            bundles.find_bundles(*stray, 1, N_SCRIPT, no_unit, 0, 3, 0, 2, 4),
            index.bundles_device(d_rows.data_ptr(), 8, 1, d_map.data_ptr(), 0, 3, 0, 2, 4)):
        assert len(units) == 0 and len(sets) == 0
        assert levels.tolist() == [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0),
                                   (5, 0, 0, NONE, NONE)]


def test_refusals(index):
    from fandom_search_amd.engine import torch_ready
    cols, n_works = quoting([[0, 1, 2]] * 4, seed=3)
    unit_of = unit_map(3)

    def refused(c, n_works=n_works, unit_of=unit_of, n_units=3, m=WIDTH, a=2, k=4,
                code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            bundles.find_bundles(*c, n_works, N_SCRIPT, unit_of, n_units, m, 0, a, k)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.bundles_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                 n_units, m, 0, a, k)
        assert e.value.code == code
    refused(cols, m=0)
    refused(cols, a=0)
    refused(cols, k=1)
    refused(cols, k=9)
    refused(cols, n_works=int(cols[0].max()))              # a work >= n_works
    fan = cols[1].copy()
    at = int(np.nonzero(cols[0][1:] == cols[0][:-1])[0][0])    # two records of one work
    fan[at] = fan[at + 1] + 1
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    bad = unit_of.copy()
    bad[N_SCRIPT - 1] = 3                                  # neither below n_units nor none
    refused(cols, unit_of=bad)
    check(index, cols, n_works, unit_of, 3)                # and the same columns are accepted


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("source,case,by,m,g,k,a,size,every", mbg.CASES)
def test_command_on_the_golden_inputs(tmp_path, source, case, by, m, g, k, a, size, every,
                                      reader):
    src = os.path.join(GOLDEN, source)
    prefix = str(tmp_path / "p")
    assert main(["bundles", src, "-o", prefix, "--by", by, "--min-words", str(m),
                 "--max-gap", str(g), "--min-works", str(k), "--min-all", str(a),
                 "--max-size", str(size), "--reader", reader] + (["--all"] if every else [])) == 0
    got = tuple(open(p, "rb").read() for p in bundles.output_names(src, prefix))
    for name, part in zip(mbg.golden_names(source, case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_command_by_character_the_default_prefix_and_the_cap(tmp_path):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, mbg.CONTRAST), src)
    assert main(["bundles", src, "--by", "character", "--min-all", "3"]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        want = br.bundles_csv(fh.read(), "character", min_all=3)
    for path, text in zip(bundles.output_names(src), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[0].count("\r\n") > 1
    with environment("FS_BUNDLES_MAX_SETS", 3):
        with pytest.raises(SystemExit) as e:
            main(["bundles", src, "-o", str(tmp_path / "capped"), "--min-all", "2"])
    line = str(e.value.code)
    assert line.startswith("ao3.py bundles: error: ") and "level 2 has 17" in line
    assert "\n" not in line and not os.path.exists(str(tmp_path / "capped-bundles.csv"))
