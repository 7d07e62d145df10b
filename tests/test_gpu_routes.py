"""`routes` on the GPU: fs_routes and fs_routes_rows against the restated contract
(tests/routes_restated.py), every field of every unit, level and route compared for equality,
the reserved words too, under FS_ROUTES_SLICE_WORDS at its default and at 1, 2 and 64; numbers
of positions around a word, a wave of words and a slice; works that end on a word's last bit,
works longer than slices; every skip at its bound and one beyond it; returning units; numbers
of extensions around a work item and of units; the cap on a level, the growing buffer, length 2
under --max-skip 0 against fs_transitions; `ao3.py routes` byte for byte against the committed
files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, routes, synth, transitions
from fandom_search_amd.cli import main
from tests import routes_restated as rr
from tests.golden import make_routes_golden as mrg
from tests.test_gpu_bundles import environment
from tests.test_gpu_companions import on_device
from tests.test_gpu_pairs import from_spans
from tests.test_routes_host import as_records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
# fs_routes.hip: 64-bit words of a slice by default, extensions of a route per work item
SLICE = 256
PIECE = 64
SLICES = (None, 1, 2, 64)   # FS_ROUTES_SLICE_WORDS: unset, and the three the tests set
N_SCRIPT = 3000             # of the index behind fs_routes_rows; every case uses it
WIDTH = 2                   # script words of a unit, and of every passage
NO_UNIT = 2600              # a passage here has no unit
DTYPES = (abi.ROUTE_UNIT_DTYPE, abi.ROUTE_LEVEL_DTYPE, abi.ROUTE_DTYPE)


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def unit_map(n_units):
    """Unit u is the script words WIDTH u .. WIDTH u + WIDTH - 1; the words behind have none."""
    o = np.arange(N_SCRIPT)
    assert n_units * WIDTH <= NO_UNIT
    return np.where(o // WIDTH < n_units, o // WIDTH, NONE).astype(np.uint32)


def quoting(works):
    """The columns of works given as the units their passages quote, in order; None is a
    passage without a unit, an empty list a work without records."""
    return from_spans([[(NO_UNIT if u is None else int(u) * WIDTH, WIDTH) for u in seq]
                       for seq in works])


def positions(works):
    """E: the elements of the collapsed sequences of two or more."""
    lengths = [len(rr.collapse([u for u in seq if u is not None])) for seq in works]
    return sum(n for n in lengths if n >= 2)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names if len(a) else ():            # (the reserved words, 0, too)
            bad = np.nonzero((a[name] != b[name]).reshape(len(a), -1).any(axis=1))[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def check(index, works, n_units, skip=NONE, a=2, k=4, slices=SLICES, unit_of=None):
    """Both entry points under every slice size against the oracle; the oracle's records."""
    from fandom_search_amd.engine import torch_ready
    cols = quoting(works)
    unit_of = unit_map(n_units) if unit_of is None else unit_of
    recs = list(zip(*(c.tolist() for c in cols)))
    want = as_records(*rr.routes(recs, len(works), N_SCRIPT, unit_of.tolist(), n_units, WIDTH, 0,
                                 skip, a, k))
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    for words in slices:
        with environment("FS_ROUTES_SLICE_WORDS", SLICE if words is None else words):
            got = routes.find_routes(*cols, len(works), N_SCRIPT, unit_of, n_units, WIDTH, 0,
                                     skip, a, k)
            assert_equal(got, want)
            dev = index.routes_device(d_rows.data_ptr(), len(cols[0]), len(works),
                                      d_map.data_ptr(), n_units, WIDTH, 0, skip, a, k)
            assert_equal(dev, want)
    got = routes.find_routes(*cols, len(works), N_SCRIPT, unit_of, n_units, WIDTH, 0,
                             None if skip == NONE else skip, a, k)     # the switch unset
    assert_equal(got, want)
    return want


def random_works(rng, n_units, total, longest=40):
    """Works of 2 .. longest elements, a few of one element or none between them, with exactly
    `total` positions."""
    works, left = [], total
    while left:
        n = left if left <= 3 else min(int(rng.integers(2, longest + 1)), left - 2)
        seq = [int(rng.integers(0, n_units))]
        while len(seq) < n:
            u = int(rng.integers(0, n_units))
            if u != seq[-1]:
                seq.append(u)
        works.append(seq)
        left -= n
        if rng.random() < 0.2:
            works.append([int(rng.integers(0, n_units))] if rng.random() < 0.5 else [])
    assert positions(works) == total
    return works


# ---- sizes ------------------------------------------------------------------------------

@pytest.mark.parametrize("total", [63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385])
@pytest.mark.parametrize("skip", [NONE, 1])
def test_positions_around_a_word_a_wave_and_a_slice(index, total, skip):
    rng = np.random.default_rng(total)
    works = random_works(rng, 3, total)
    units, levels, found = check(index, works, 3, skip, a=max(2, total // 200), k=3)
    assert units["works"].min() > 0 and levels["frequent"][0] == 6 and len(found) > 6


def filler(n, first=2):
    """n elements that are neither unit 0 nor unit 1."""
    return [first + (t & 1) for t in range(n)]


@pytest.mark.parametrize("last_bit", [63, 64 * 64 - 1, SLICE * 64 - 1])
def test_a_work_that_ends_on_the_last_bit_and_a_head_on_it(index, last_bit):
    """A work whose last element, unit 0, is bit 63 of a word (of a wave's last word, of a
    slice's last word) and the next work starts with unit 1: no route (0, 1) across the two.
    Then the same with a work of two in front, so that the head is the last bit."""
    front = filler(last_bit) + [0]
    nxt = [1, 2, 0, 1]
    works = [front[:len(front) // 2], front[len(front) // 2:], nxt, [3, 1], [0, 3]]
    assert positions(works[:2]) == last_bit + 1
    for skip in (NONE, 0):
        units, levels, found = check(index, works, 4, skip, a=1, k=2)
        r01 = found[(found["units"][:, :2] == [0, 1]).all(axis=1) & (found["length"] == 2)]
        assert len(r01) == 1 and r01[0]["works"] == 1 and r01[0]["first_work"] == 2
    shifted = [front[:len(front) // 2], front[len(front) // 2:-1], [0, 1], [1, 0, 1]]
    assert positions(shifted[:2]) == last_bit                 # the head of [0, 1] is the last bit
    units, levels, found = check(index, shifted, 4, NONE, a=1, k=2)
    r01 = found[(found["units"][:, :2] == [0, 1]).all(axis=1) & (found["length"] == 2)]
    assert r01[0]["works"] == 2 and r01[0]["first_work"] == 2
    r10 = found[(found["units"][:, :2] == [1, 0]).all(axis=1) & (found["length"] == 2)]
    assert r10[0]["works"] == 1 and r10[0]["first_work"] == 3


def test_a_work_through_three_slices(index):
    """One work from the middle of the first default slice to the middle of the third: the
    second has no head.  Units 0 and 1 once each, a slice apart, are the only (0, 1)."""
    n = 2 * SLICE * 64 + 300
    long_work = filler(n)
    long_work[100] = 0
    long_work[n - 50] = 1
    works = [filler(SLICE * 32), long_work, [1, 3, 0], [2, 3]]
    units, levels, found = check(index, works, 4, NONE, a=1, k=2)
    r01 = found[(found["units"][:, :2] == [0, 1]).all(axis=1) & (found["length"] == 2)]
    assert len(r01) == 1 and r01[0]["works"] == 1 and r01[0]["first_work"] == 1
    assert r01[0]["closed"] == 0 and r01[0]["forward"] > 0    # (0, 1, 2) in the same work
    bounded = check(index, works, 4, 63, a=1, k=2)[2]          # and no (0, 1) within 64
    assert not ((bounded["units"][:, :2] == [0, 1]).all(axis=1) & (bounded["length"] == 2)).any()


# ---- the skip ---------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [0, 1, 62, 63, NONE])
def test_two_units_at_the_bound_and_one_beyond(index, skip):
    """Unit 0 on the bits 62, 63 and 0 of a word, unit 1 exactly max_skip + 1 behind it and one
    further; unit 0 as a work's last element with unit 1 within reach in the next work."""
    D = 70 if skip == NONE else skip + 1
    works, reached, at = [], 0, 0
    for bit in (62, 63, 64):
        for apart in (D, D + 1):
            pad = (bit - at) % 64 + 64                        # the work in front
            works.append(filler(pad))
            works.append([0] + filler(apart - 1) + [1] + filler(2))
            at += pad + apart + 3
            reached += apart == D or skip == NONE
    pad = (63 - at) % 64 + 64
    works += [filler(pad - 1) + [0], [2, 1, 3], [1, 2]]       # 0 on bit 63, the work ends there
    units, levels, found = check(index, works, 4, skip, a=1, k=2)
    r01 = found[(found["units"][:, :2] == [0, 1]).all(axis=1) & (found["length"] == 2)]
    assert len(r01) == 1 and r01[0]["works"] == reached and r01[0]["first_work"] == 1
    assert reached == (6 if skip == NONE else 3)


def test_returning_units_a_collapse_and_a_passage_without_a_unit(index):
    works = [[0, 1, 0, 1], [0, 1, 0], [0, 0, 0, 1], [0, None, 0, 1], [1, None, None, 1],
             [None, 0, None, 1, 0, 1], [None], [0, None]]
    assert positions(works) == 4 + 3 + 2 + 2 + 0 + 4 + 0 + 0
    for skip in (NONE, 0):
        units, levels, found = check(index, works, 2, skip, a=1, k=4)
        got = {tuple(r["units"][:r["length"]]): int(r["works"]) for r in found}
        assert got == {(0, 1): 5, (1, 0): 3, (0, 1, 0): 3, (1, 0, 1): 2, (0, 1, 0, 1): 2}
        assert units["works"].tolist() == [5, 5] and units["routes"].tolist() == [5, 5]
        assert levels["frequent"].tolist() == [2, 2, 1, 0]     # no (1, 0, 1, 0, 1)
    units, levels, found = check(index, works, 2, NONE, a=3, k=4)
    assert [int(r["closed"]) for r in found] == [1, 0, 1]      # (1, 0) has the works of (0, 1, 0)


# ---- extensions, units, length ----------------------------------------------------------

@pytest.mark.parametrize("group", [1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 2])
def test_a_route_with_so_many_extensions(index, group):
    """Unit 0, then one of the units 1 .. group, two works each: unit 0 has `group`
    extensions at level 2, all frequent; 130 are three work items."""
    works = [[0, x] for x in range(1, group + 1) for _ in range(2)]
    units, levels, found = check(index, works, group + 2, NONE, a=2, k=3, slices=(None, 1))
    assert levels["candidates"][0] == (group + 1) * group
    assert levels["frequent"].tolist() == [group, 0, 0]
    assert (found["units"][:, 1] == np.arange(1, group + 1)).all()
    assert (found["works"] == 2).all() and (found["prefix_works"] == 2 * group).all()
    assert tuple(units[group + 1]) == (0, 0, 0, 0)
    assert tuple(units[0]) == (2 * group, group, 2, 0)


@pytest.mark.parametrize("n_units", [1, 2, 64, 65, 513])
def test_so_many_units(index, n_units):
    rng = np.random.default_rng(n_units)
    hot = np.unique(np.linspace(0, n_units - 1, min(5, n_units)).astype(int))
    works = []
    for _ in range(60):
        seq = rng.choice(hot, size=min(3, len(hot)), replace=False).tolist()
        seq.insert(int(rng.integers(0, len(seq) + 1)), int(rng.integers(0, n_units)))
        works.append(seq)
    units, levels, found = check(index, works, n_units, NONE, a=3, k=3, slices=(None, 2))
    if n_units == 1:
        assert not units["works"].any() and not levels["candidates"].any() and not len(found)
    else:
        assert len(found) > 0 and found["units"][:, :2].max() == n_units - 1


def test_a_route_of_nine_units_under_max_length_eight(index):
    works = [list(range(9))] * 3 + [[8, 0], [4]]
    units, levels, found = check(index, works, 10, NONE, a=3, k=8, slices=(None, 1))
    assert levels["length"].tolist() == list(range(2, 10))
    assert levels["frequent"].tolist() == [36, 84, 126, 126, 84, 36, 9, 1]   # level 9: mined
    # closed: nothing frequent in front or behind, so from unit 0 to unit 8, any k - 2 between
    assert levels["closed"].tolist() == [1, 7, 21, 35, 35, 21, 7, NONE]
    eight = found[found["length"] == 8]
    whole = eight[(eight["units"] == np.arange(8)).all(axis=1)]
    assert len(whole) == 1 and whole[0]["closed"] == 0 and whole[0]["forward"] == 1
    run = check(index, works, 10, 0, a=3, k=8, slices=(None,))
    assert run[1]["frequent"].tolist() == [8, 7, 6, 5, 4, 3, 2, 1]
    L = _lib.load()
    ms = (C.c_double * abi.FS_ROUTES_TIMES)()
    assert L.fs_routes_times(ms) == abi.FS_OK
    assert ms[0] > 0 and ms[3] > 0 and ms[42] >= ms[0] + ms[2] + ms[3]


# ---- the cap, the growing buffer, the refusals -------------------------------------------

def _call(L, cols, n_works, unit_of, n_units, skip, a, k, units, levels, found, cap, n):
    return L.fs_routes(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                       abi.ptr(cols[2], C.c_uint32), len(cols[0]), n_works, N_SCRIPT,
                       abi.ptr(unit_of, C.c_uint32), n_units, WIDTH, 0, skip, a, k,
                       units.ctypes.data_as(C.c_void_p), levels.ctypes.data_as(C.c_void_p),
                       found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


def oracle(cols, n_works, unit_of, n_units, skip, a, k):
    recs = list(zip(*(c.tolist() for c in cols)))
    return as_records(*rr.routes(recs, n_works, N_SCRIPT, unit_of.tolist(), n_units, WIDTH, 0,
                                 skip, a, k))


def test_a_level_one_above_the_cap_is_refused_and_one_at_it_is_not(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    works = [[0, 1, 2, 3, 4]] * 2
    cols = [np.ascontiguousarray(c) for c in quoting(works)]
    unit_of = unit_map(5)
    want = oracle(cols, 2, unit_of, 5, NONE, 2, 3)
    assert want[1]["candidates"].tolist() == [20, 10, 5]        # the largest: level 2
    L = _lib.load()
    units = np.ones(5, dtype=abi.ROUTE_UNIT_DTYPE)
    levels = np.ones(3, dtype=abi.ROUTE_LEVEL_DTYPE)
    found = np.ones(40, dtype=abi.ROUTE_DTYPE)
    before = [x.tobytes() for x in (units, levels, found)]
    n = C.c_uint64(0)
    d_rows, d_map = on_device(cols, unit_of)
    d_out = [torch.ones(len(x) * x.dtype.itemsize, dtype=torch.uint8, device="cuda")
             for x in (units, levels, found)]
    torch_ready()
    with environment("FS_ROUTES_MAX_SETS", 19):
        assert _call(L, cols, 2, unit_of, 5, NONE, 2, 3, units, levels, found, 40, n) == \
            abi.FS_E_UNSUPPORTED
        text = L.fs_last_error().decode()
        assert "level 2 has 20 candidate routes" in text
        assert "--min-all" in text and "--max-length" in text
        for x, was in zip((units, levels, found), before):     # the output buffers untouched
            assert x.tobytes() == was
        with pytest.raises(_lib.FsError) as e:
            index.routes_device(d_rows.data_ptr(), len(cols[0]), 2, d_map.data_ptr(), 5, WIDTH,
                                0, NONE, 2, 3, out_ptrs=[t.data_ptr() for t in d_out], cap=40)
        assert e.value.code == abi.FS_E_UNSUPPORTED
        assert all(bool((t == 1).all()) for t in d_out)
    with environment("FS_ROUTES_MAX_SETS", 20):
        assert _call(L, cols, 2, unit_of, 5, NONE, 2, 3, units, levels, found, 40, n) == abi.FS_OK
    assert n.value == 20
    assert_equal((units, levels, found[:20]), want)


def test_capacity_grows_from_one(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    rng = np.random.default_rng(8)
    works = random_works(rng, 5, 300, longest=8)
    cols = [np.ascontiguousarray(c) for c in quoting(works)]
    unit_of = unit_map(5)
    want = oracle(cols, len(works), unit_of, 5, NONE, 2, 3)
    k = len(want[2])
    assert k > 10
    L = _lib.load()
    units = np.zeros(5, dtype=abi.ROUTE_UNIT_DTYPE)
    levels = np.zeros(3, dtype=abi.ROUTE_LEVEL_DTYPE)
    found = np.zeros(k, dtype=abi.ROUTE_DTYPE)
    n = C.c_uint64(0)
    for cap in (1, k - 1, 0):
        units[:] = 0
        levels[:] = 0
        assert _call(L, cols, len(works), unit_of, 5, NONE, 2, 3, units, levels, found, cap,
                     n) == abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((units, levels, want[2]), want)       # the units and levels are complete
        assert not found.view(np.uint8).any()              # the routes untouched
    assert _call(L, cols, len(works), unit_of, 5, NONE, 2, 3, units, levels, found, k, n) == \
        abi.FS_OK
    assert_equal((units, levels, found), want)
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    args = (d_rows.data_ptr(), len(cols[0]), len(works), d_map.data_ptr(), 5, WIDTH, 0, NONE, 2,
            3)
    assert_equal(index.routes_device(*args, cap=1), want)  # grown by the wrapper
    d_out = [torch.zeros(len(x) * x.dtype.itemsize, dtype=torch.uint8, device="cuda")
             for x in (units, levels, found)]
    torch_ready()
    ptrs = [t.data_ptr() for t in d_out]
    with pytest.raises(_lib.FsError) as e:
        index.routes_device(*args, out_ptrs=ptrs, cap=1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_out[0].cpu().numpy().view(abi.ROUTE_UNIT_DTYPE) == want[0]).all()
    assert (d_out[1].cpu().numpy().view(abi.ROUTE_LEVEL_DTYPE) == want[1]).all()
    assert not d_out[2].cpu().numpy().any()
    assert index.routes_device(*args, out_ptrs=ptrs, cap=k) == k
    assert (d_out[2].cpu().numpy().view(abi.ROUTE_DTYPE) == want[2]).all()
    # no records, and no units, on the device
    assert index.routes_device(d_rows.data_ptr(), 0, len(works), d_map.data_ptr(), 5, WIDTH, 0,
                               NONE, 2, 3, out_ptrs=ptrs, cap=k) == 0
    assert not d_out[0].cpu().numpy().any()
    assert index.routes_device(*args[:4], 0, WIDTH, 0, NONE, 2, 3, out_ptrs=ptrs, cap=k) == 0


def test_no_records_no_units_and_no_sequence_of_two(index):
    units, levels, found = check(index, [[], [], []], 5, slices=(None,))
    assert units.tolist() == [(0, 0, 0, 0)] * 5 and len(found) == 0
    assert levels.tolist() == [(2, 0, 0, 0, 0), (3, 0, 0, 0, 0), (4, 0, 0, 0, 0),
                               (5, 0, 0, NONE, 0)]
    works = [[0, 1]] * 3
    units, levels, found = check(index, works, 0, unit_of=np.full(N_SCRIPT, NONE, np.uint32),
                                 slices=(None,))
    assert len(units) == 0 and len(found) == 0
    units, levels, found = check(index, [[0], [1, 1], [None, 2]], 5, slices=(None,))
    assert units.tolist() == [(0, 0, 0, 0)] * 5 and len(found) == 0


def test_refusals(index):
    from fandom_search_amd.engine import torch_ready
    works = [[0, 1, 2]] * 4
    cols = quoting(works)
    unit_of = unit_map(3)

    def refused(c, n_works=4, unit_of=unit_of, n_units=3, m=WIDTH, skip=NONE, a=2, k=4,
                code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            routes.find_routes(*c, n_works, N_SCRIPT, unit_of, n_units, m, 0, skip, a, k)
        assert e.value.code == code
        d_rows, d_map = on_device(c, unit_of)
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            index.routes_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                n_units, m, 0, skip, a, k)
        assert e.value.code == code
    refused(cols, m=0)
    refused(cols, a=0)
    refused(cols, k=1)
    refused(cols, k=9)
    refused(cols, skip=64)
    refused(cols, skip=NONE - 1)
    refused(cols, n_works=int(cols[0].max()))              # a work >= n_works
    fan = cols[1].copy()
    fan[0] = fan[1] + 1
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    bad = unit_of.copy()
    bad[N_SCRIPT - 1] = 3                                  # neither below n_units nor none
    refused(cols, unit_of=bad)
    check(index, works, 3, slices=(None,))                 # and the same columns are accepted


def test_length_two_without_a_skip_is_the_cells_of_transitions(index):
    rng = np.random.default_rng(12)
    works = random_works(rng, 7, 900, longest=12)
    for seq in works[::3]:                                 # passages that repeat and have no unit
        seq.insert(len(seq) // 2, seq[len(seq) // 2 - 1] if len(seq) > 1 else None)
        seq.append(None)
    cols = quoting(works)
    unit_of = unit_map(7)
    for bar in (1, 2, 5):
        units, levels, found = routes.find_routes(*cols, len(works), N_SCRIPT, unit_of, 7, WIDTH,
                                                  0, 0, bar, 2)
        tu, cells = transitions.find_transitions(*cols, len(works), N_SCRIPT, unit_of, 7, WIDTH,
                                                 0, NONE, 1, bar, 0)
        cells = cells[cells["a"] != cells["b"]]
        two = found[found["length"] == 2]
        assert len(two) == len(cells) == len(found) > 0
        assert (two["units"][:, 0] == cells["a"]).all() and (two["units"][:, 1] == cells["b"]).all()
        assert (two["works"] == cells["works"]).all()
        assert (two["first_work"] == cells["first_work"]).all()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("source,case,by,m,g,k,a,length,skip,every", mrg.CASES)
def test_command_on_the_golden_inputs(tmp_path, source, case, by, m, g, k, a, length, skip,
                                      every):
    src = os.path.join(GOLDEN, source)
    files = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / reader)
        assert main(["routes", src, "-o", prefix, "--by", by, "--min-words", str(m),
                     "--max-gap", str(g), "--min-works", str(k), "--min-all", str(a),
                     "--max-length", str(length), "--reader", reader]
                    + ([] if skip is None else ["--max-skip", str(skip)])
                    + (["--all"] if every else [])) == 0
        files[reader] = tuple(open(p, "rb").read() for p in routes.output_names(src, prefix))
        for name, part in zip(mrg.golden_names(source, case), files[reader]):
            with open(os.path.join(GOLDEN, name), "rb") as fh:
                assert part == fh.read(), name
    assert files["device"] == files["python"]


def test_a_route_planted_in_forty_works_is_one_row_and_the_cap_one_line(tmp_path):
    import csv
    rng = np.random.default_rng(40)
    lines = {0: "we meet in the cantina", 1: "stay on target now luke", 2: "here is your medal sir",
             3: "these are not the droids", 4: "it is a trap admiral"}
    script, at = [], {}
    for u, text in lines.items():
        at[u] = len(script)
        script += [(w, "C%d" % u, str(u + 1)) for w in text.split()] + [("pad", "N", "9")]
    src = str(tmp_path / "m.csv")
    with open(os.path.join(GOLDEN, mrg.TRANSITIONS), newline="", encoding="utf-8") as fh:
        head = next(csv.reader(fh))
    with open(src, "w", newline="", encoding="utf-8") as fh:
        out = csv.writer(fh)
        out.writerow(head)
        for w in range(46):
            order = [0, 1, 2] if w < 40 else rng.permutation([3, 4, 2]).tolist()
            fan = 0
            for u in order:
                for t in range(5):
                    o = at[u] + t
                    word, who, scene = script[o]
                    out.writerow(["w%02d.txt" % w, fan, word, 100 + o, o, word, 300 + o, who,
                                  scene, "0.0", "0", "0.0"])
                    fan += 1
                fan += 7
    assert main(["routes", src, "--min-words", "5", "--min-all", "40", "--max-length", "3",
                 "--max-skip", "0"]) == 0
    with open(routes.output_names(src)[0], newline="", encoding="utf-8") as fh:
        rows = list(csv.reader(fh))
    assert len(rows) == 2 and rows[1][1:4] == ["3", "1 > 2 > 3", "40"]
    assert rows[1][6] == "forward" and rows[1][7] == "1"
    with environment("FS_ROUTES_MAX_SETS", 3):
        with pytest.raises(SystemExit) as e:
            main(["routes", src, "-o", str(tmp_path / "capped"), "--min-words", "5",
                  "--min-all", "2"])
    line = str(e.value.code)
    assert line.startswith("ao3.py routes: error: ") and "level 2 has 20" in line
    assert "\n" not in line and not os.path.exists(str(tmp_path / "capped-routes.csv"))
