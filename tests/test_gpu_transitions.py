"""`transitions` on the GPU: fs_transitions and fs_transitions_rows against the restated contract
(tests/transitions_restated.py), every field of every unit and cell compared for equality,
every case down each counting path in turn (FS_TRANSITIONS_DENSE, FS_TRANSITIONS_HASH_BITS);
sequence lengths, numbers of units and of successors around every size the kernels treat
differently; `ao3.py transitions` byte for byte against the committed files.

Passages here are WORDS records long (--min-words WORDS); unit u is the script words
[WIDTH u, WIDTH u + WIDTH), the words behind the last unit have none."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, synth, transitions
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests import transitions_restated as tr
from tests.golden import make_transitions_golden as mtg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
N_SCRIPT = 3000          # of the index behind fs_transitions_rows; every case uses it
WORDS = 2
WIDTH = 4
FAN_GAP = 3              # fan words between two passages of a work: they never join
NO_UNIT = N_SCRIPT - 10  # a script word behind every unit
DENSE = 64               # include/fandom_search.h: units of the dense class at most
LONG = 64                # fs_transitions.hip: kept cells of a unit ranked by one lane at most
# (FS_TRANSITIONS_DENSE, FS_TRANSITIONS_HASH_BITS)
PATHS = {"default": (None, None), "hashed": ("0", None), "bits4": (None, "4"),
         "bits0": (None, "0")}


@pytest.fixture(params=list(PATHS), ids=list(PATHS))
def path(request, monkeypatch):
    for name, value in zip(("FS_TRANSITIONS_DENSE", "FS_TRANSITIONS_HASH_BITS"),
                           PATHS[request.param]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def unit_map(n_units):
    o = np.arange(N_SCRIPT)
    assert n_units * WIDTH <= NO_UNIT
    return np.where(o // WIDTH < n_units, o // WIDTH, NONE).astype(np.uint32)


def placed(works):
    """Columns (work, fan_ix, orig_ix) of {work: [(fan_first, orig_first), ...]}, passages of
    WORDS records."""
    cols = [[], [], []]
    for w in sorted(works):
        for fan, orig in works[w]:
            cols[0] += [w] * WORDS
            cols[1] += range(fan, fan + WORDS)
            cols[2] += range(orig, orig + WORDS)
    return tuple(np.asarray(c, dtype=np.uint32) for c in cols)


def layout(works, gap=FAN_GAP):
    """Columns of {work: [unit or None, ...]}: the passages of a work one behind another, `gap`
    fan words between them, each at the first word of its unit (None: at a word of no unit)."""
    return placed({w: [((WORDS + gap) * k, NO_UNIT if u is None else WIDTH * u + k % 2)
                       for k, u in enumerate(units)] for w, units in works.items()})


def oracle(cols, n_works, unit_of, n_units, **options):
    recs = list(zip(*(c.tolist() for c in cols)))
    units, found = tr.transitions(recs, n_works, N_SCRIPT, np.asarray(unit_of).tolist(), n_units,
                                  WORDS, **options)
    u = np.array([tuple(r[k] for k in tr.UNIT_KEYS) for r in units],
                 dtype=abi.TRANSITION_UNIT_DTYPE)
    c = np.array([tuple(r[k] for k in tr.CELL_KEYS) for r in found], dtype=abi.TRANSITION_DTYPE)
    return u, c


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.TRANSITION_UNIT_DTYPE, abi.TRANSITION_DTYPE)):
        assert a.dtype == dt and len(a) == len(b), (len(a), len(b))
        for name in dt.names:
            bad = np.flatnonzero(a[name] != b[name])
            assert not len(bad), (name, bad[:5], a[name][bad[:5]], b[name][bad[:5]])
    units, cells = got
    assert units["starts"].sum() == units["ends"].sum()
    assert units["steps_out"].sum() == units["steps_in"].sum()
    keys = cells["a"].astype(np.int64) << 32 | cells["b"]
    assert (np.diff(keys) > 0).all()                           # (a, b) ascending, no cell twice


def on_device(cols, unit_of):
    """(rows tensor, unit map tensor) in HBM."""
    import torch
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name][:len(col)] = col
    return (torch.from_numpy(rows.view(np.uint8)).to("cuda"),
            torch.from_numpy(np.ascontiguousarray(unit_of, dtype=np.uint32)).to("cuda"))


def check(index, cols, n_works, n_units, unit_of=None, want=None, max_gap=0, within=NONE,
          min_steps=1, min_step_works=1, min_share=0):
    """Both entry points against the oracle; the host entry point's result."""
    from fandom_search_amd.engine import torch_ready
    unit_of = unit_map(n_units) if unit_of is None else unit_of
    options = dict(max_gap=max_gap, within=within, min_steps=min_steps,
                   min_step_works=min_step_works, min_share=min_share)
    if want is None:
        want = oracle(cols, n_works, unit_of, n_units, **options)
    got = transitions.find_transitions(*cols, n_works, N_SCRIPT, unit_of, n_units, WORDS,
                                       **options)
    assert_equal(got, want)
    d_rows, d_map = on_device(cols, unit_of)
    torch_ready()
    dev = index.transitions_device(d_rows.data_ptr(), len(cols[0]), n_works, d_map.data_ptr(),
                                   n_units, WORDS, **options)
    assert_equal(dev, want)
    return got


# ---- one work of p passages: the neighbour look-up on lane, wave and workgroup edges ------

P = [1, 2, 63, 64, 65, 255, 256, 257, 300]
KINDS = {"one": (1, lambda p: [0] * p), "two": (2, lambda p: [k % 2 for k in range(p)]),
         "cycle7": (7, lambda p: [k % 7 for k in range(p)]),
         "random5": (5, lambda p: np.random.default_rng(p).integers(0, 5, p).tolist())}


@functools.lru_cache(maxsize=None)
def one_work(kind, p):
    n_units, units = KINDS[kind]
    cols = layout({0: units(p)})
    return cols, n_units, oracle(cols, 1, unit_map(n_units), n_units, min_step_works=1)


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_work_of_p_passages(index, path, kind, p):
    cols, n_units, want = one_work(kind, p)
    units, cells = check(index, cols, 1, n_units, want=want)
    assert units["passages"].sum() == p and cells["steps"].sum() == p - 1
    assert units["starts"].sum() == 1 and (cells["works"] == 1).all()
    if kind == "two" and p > 2:
        assert cells["steps"].tolist() == [p // 2, (p - 1) // 2]


# ---- many works: no step crosses a work ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def many_works(shift):
    """Works of 1..3 passages, 8 passages to every four works, behind a first work of `shift`
    passages: at shift 0 a work ends at sequence elements 63 and 255, at 1 and 2 a work lies
    across them; then 70 works of one passage."""
    sizes = ([shift] if shift else []) + [1, 2, 3, 2] * 70 + [1] * 70
    rng = np.random.default_rng(shift)
    works = {2 * w: rng.integers(0, 6, size).tolist() for w, size in enumerate(sizes)}
    cols = layout(works)
    n_works = 2 * len(sizes)
    return cols, n_works, len(sizes), oracle(cols, n_works, unit_map(6), 6, min_step_works=1)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_many_works_with_a_boundary_at_and_across_lane_63_and_element_255(index, path, shift):
    cols, n_works, n_active, want = many_works(shift)
    units, cells = check(index, cols, n_works, 6, want=want)
    assert units["starts"].sum() == units["ends"].sum() == n_active
    assert units["passages"].sum() - n_active == cells["steps"].sum()     # a work of k: k - 1
    assert units["passages"].sum() > 600


# ---- the number of units: the class bound and both sides ----------------------------------

def random_works(n_works, most, n_units, seed, unitless=0.1):
    rng = np.random.default_rng(seed)
    works = {}
    for w in range(n_works):
        units = rng.integers(0, n_units, int(rng.integers(0, most + 1))).tolist()
        works[w] = [None if rng.random() < unitless else u for u in units]
    return layout(works)


@pytest.mark.parametrize("n_units", [1, 2, DENSE - 1, DENSE, DENSE + 1, 300])
def test_units_around_the_dense_class(index, path, n_units):
    cols = random_works(120, 12, n_units, seed=n_units)
    units, cells = check(index, cols, 120, n_units)
    assert len(cells) > 0 and units["works"].sum() > 0
    check(index, cols, 120, n_units, min_step_works=2, min_share=3)


# ---- one hot cell ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hot(n_units):
    # 700 works looping in the last unit: 7 steps each, 8 for the first hundred: 5 000 steps
    u = n_units - 1
    works = {w + 3: [u] * (9 if w < 100 else 8) for w in range(700)}
    cols = layout(works)
    return cols, oracle(cols, 703, unit_map(n_units), n_units, min_step_works=1)


@pytest.mark.parametrize("n_units", [2, DENSE + 1])
def test_five_thousand_steps_of_700_works_into_one_cell(index, path, n_units):
    cols, want = hot(n_units)
    units, cells = check(index, cols, 703, n_units, want=want)
    assert cells.tolist() == [(n_units - 1, n_units - 1, 5000, 0, 700, 3, 5000, 5000)]
    assert not units["passages"][:n_units - 1].any()
    assert tuple(units[n_units - 1]) == (5700, 700, 700, 700, 5000, 5000, 1, 1, n_units - 1, 5000)


# ---- a unit of many successors: the wave-rank bound ---------------------------------------

@pytest.mark.parametrize("n_units,k", [(DENSE, LONG), (LONG + 1, LONG), (LONG + 2, LONG + 1),
                                       (201, 200)])
def test_a_unit_of_many_successors_comes_out_in_ascending_b(index, path, n_units, k):
    # unit 0 to each of the last k units, the works in a shuffled order; some steps twice
    order = np.random.default_rng(k).permutation(k)
    works = {w: [0, n_units - k + int(b)] * (1 + w % 2) for w, b in enumerate(order)}
    units, cells = check(index, layout(works), k, n_units)
    out = cells[cells["a"] == 0]
    assert units["successors"][0] == k == len(out)
    assert out["b"].tolist() == list(range(n_units - k, n_units))
    if n_units > k:                                            # (else a loop 0 -> 0 is among them)
        assert units["best_next"][0] == n_units - k + int(order[1::2].min())
        assert units["best_steps"][0] == 2


# ---- within ---------------------------------------------------------------------------------

def test_within_at_one_below_and_one_above_the_bound(index, path):
    # work 0: 5 fan words between its passages, work 1: 6, work 2: 4
    works = {0: [(0, 0), (7, 4)], 1: [(0, 0), (8, 4)], 2: [(0, 0), (6, 4)]}
    for within, steps in ((3, 0), (4, 1), (5, 2), (6, 3), (7, 3), (NONE, 3), (NONE - 1, 3)):
        units, cells = check(index, placed(works), 3, 2, within=within)
        assert cells["steps"].sum() == steps
        assert units["ends"].tolist() == [0, 3] and units["starts"].tolist() == [3, 0]


def test_within_zero_with_passages_that_touch(index, path):
    # fan words 0..1 then 2..3: nothing between; the script jumps, so --max-gap 1 joins nothing.
    # Work 1 repeats fan word 1: the passages share it.  Work 2 leaves one word between
    works = {0: [(0, 0), (2, 40)], 1: [(0, 0), (1, 40)], 2: [(0, 0), (3, 40)]}
    units, cells = check(index, placed(works), 3, 11, max_gap=1, within=0)
    assert cells.tolist() == [(0, 10, 2, 2, 2, 0, 2, 2)]
    units, cells = check(index, placed(works), 3, 11, max_gap=1, within=1)
    assert cells["steps"].tolist() == [3]


def test_within_next_to_the_largest_fan_index(index, path):
    top = 0xFFFFFFFF - WORDS                  # its passage ends at fan word 2^32 - 2
    works = {0: [(0, 0), (top, 4)]}
    between = top - 1 - 1                     # fan words 2 .. top - 1
    for within, steps in ((NONE - 1, 1), (between, 1), (between - 1, 0), (0, 0), (NONE, 1)):
        units, cells = check(index, placed(works), 1, 2, within=within)
        assert cells["steps"].sum() == steps and units["passages"].tolist() == [1, 1]


# ---- passages without a unit ----------------------------------------------------------------

@pytest.mark.parametrize("where", ["first", "last", "middle", "all"])
def test_passages_without_a_unit(index, path, where):
    seq = {"first": [None, 0, 1, 2], "last": [0, 1, 2, None], "middle": [0, None, None, 1, 2],
           "all": [None, None, None]}[where]
    works = {0: seq, 1: [2, 1], 2: seq}
    units, cells = check(index, layout(works), 3, 3)
    if where == "all":
        only = check(index, layout({0: seq, 2: seq}), 3, 3)
        assert not any(only[0][name].any() for name in tr.UNIT_KEYS if name != "best_next")
        assert (only[0]["best_next"] == NONE).all() and len(only[1]) == 0
    else:
        assert [(c["a"], c["b"], c["steps"]) for c in cells] == [(0, 1, 2), (1, 2, 2), (2, 1, 1)]
        assert units["starts"].tolist() == [2, 0, 1] and units["ends"].tolist() == [0, 1, 2]
    # the fan words between count from the passages with a unit
    if where == "middle":
        step = WORDS + FAN_GAP
        assert check(index, layout(works), 3, 3, within=3 * step - WORDS)[1]["steps"][0] == 2
        got = check(index, layout(works), 3, 3, within=3 * step - WORDS - 1)[1]
        assert [(c["a"], c["b"]) for c in got] == [(1, 2), (2, 1)]


# ---- the keep rule ----------------------------------------------------------------------------

def keep_rule_works():
    # work 0 steps 0 -> 1 twice, works 1..3 once: 5 steps of 4 works; works 4..8 step 0 -> 2:
    # steps_out(0) = 10, each of the two cells 50 percent of it; (1, 0) is work 0's way back
    return layout(dict(enumerate([[0, 1, 0, 1]] + [[0, 1]] * 3 + [[0, 2]] * 5)))


@pytest.mark.parametrize("options,kept", [
    (dict(), [(0, 1), (0, 2), (1, 0)]),
    (dict(min_share=50), [(0, 1), (0, 2), (1, 0)]), (dict(min_share=51), [(1, 0)]),
    (dict(min_share=100), [(1, 0)]),
    (dict(min_steps=5), [(0, 1), (0, 2)]), (dict(min_steps=6), []),
    (dict(min_step_works=4), [(0, 1), (0, 2)]), (dict(min_step_works=5), [(0, 2)]),
    (dict(min_step_works=6), []), (dict(min_steps=5, min_step_works=5, min_share=50), [(0, 2)])])
def test_the_keep_rule_at_and_above_a_cell_s_figures(index, path, options, kept):
    units, cells = check(index, keep_rule_works(), 9, 3, **options)
    assert [(c["a"], c["b"]) for c in cells] == kept
    assert units["steps_out"].tolist() == [10, 1, 0] and units["steps_in"].tolist() == [1, 5, 5]
    assert units["successors"].tolist() == [sum(a == u for a, _ in kept) for u in range(3)]
    assert units["predecessors"].tolist() == [sum(b == u for _, b in kept) for u in range(3)]


def test_best_next_under_equal_steps(index, path):
    works = dict(enumerate([[1, 2], [1, 0], [1, 1]]))
    units, _ = check(index, layout(works), 3, 3)
    assert (units["best_next"][1], units["best_steps"][1]) == (0, 1)
    works = dict(enumerate([[1, 2], [1, 0], [1, 1], [1, 2], [1, 1]]))
    units, _ = check(index, layout(works), 5, 3)
    assert (units["best_next"][1], units["best_steps"][1]) == (1, 2)
    units, _ = check(index, layout(works), 5, 3, min_step_works=2)     # (1, 0) not kept
    assert (units["best_next"][1], units["successors"][1]) == (1, 2)
    assert units["best_next"][[0, 2]].tolist() == [NONE, NONE]


# ---- capacity, refusals, nothing to do ----------------------------------------------------

def _call(L, cols, n_works, unit_of, n_units, units, found, cap, n, n_rows=None,
          n_script=N_SCRIPT, m=WORDS, steps=1, step_works=1, share=0):
    return L.fs_transitions(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                            abi.ptr(cols[2], C.c_uint32),
                            len(cols[0]) if n_rows is None else n_rows, n_works, n_script,
                            abi.ptr(unit_of, C.c_uint32), n_units, m, 0, NONE, steps, step_works,
                            share, units.ctypes.data_as(C.c_void_p),
                            found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


@pytest.mark.parametrize("n_units", [20, DENSE + 6])
def test_capacity_zero_one_short_and_exact(index, path, n_units):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols = [np.ascontiguousarray(c) for c in random_works(100, 10, n_units, seed=8)]
    unit_of = unit_map(n_units)
    want = oracle(cols, 100, unit_of, n_units, min_step_works=1)
    k = len(want[1])
    assert k > 10
    L = _lib.load()
    units = np.zeros(n_units, dtype=abi.TRANSITION_UNIT_DTYPE)
    found = np.zeros(k, dtype=abi.TRANSITION_DTYPE)
    n = C.c_uint64(0)
    for cap in (k - 1, 0):
        units[:] = 0
        assert _call(L, cols, 100, unit_of, n_units, units, found, cap, n) == abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((units, want[1]), want)               # the units are complete
        assert not found["steps"].any()                    # the cells untouched
    assert _call(L, cols, 100, unit_of, n_units, units, found, k, n) == abi.FS_OK
    assert n.value == k
    assert_equal((units, found), want)
    # the caller's own device buffers
    d_rows, d_map = on_device(cols, unit_of)
    d_units = torch.zeros(n_units * 40, dtype=torch.uint8, device="cuda")
    d_cells = torch.zeros(k * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_units.data_ptr(), d_cells.data_ptr())
    args = (d_rows.data_ptr(), len(cols[0]), 100, d_map.data_ptr(), n_units, WORDS, 0, NONE, 1, 1,
            0)
    with pytest.raises(_lib.FsError) as e:
        index.transitions_device(*args, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_units.cpu().numpy().view(abi.TRANSITION_UNIT_DTYPE) == want[0]).all()
    assert not d_cells.cpu().numpy().any()
    assert index.transitions_device(*args, out_ptrs=ptrs, cap=k) == k
    assert (d_cells.cpu().numpy().view(abi.TRANSITION_DTYPE) == want[1]).all()
    # no records, and no units, on the device
    assert index.transitions_device(d_rows.data_ptr(), 0, 100, d_map.data_ptr(), n_units, WORDS,
                                    out_ptrs=ptrs, cap=k) == 0
    none = d_units.cpu().numpy().view(abi.TRANSITION_UNIT_DTYPE)
    assert (none["best_next"] == NONE).all() and not none["passages"].any()
    assert index.transitions_device(*args[:4], 0, WORDS, out_ptrs=ptrs, cap=k) == 0


def test_no_records_no_units_and_no_passages(index, path):
    empty = (np.zeros(0, np.uint32),) * 3
    none = [(0,) * 8 + (NONE, 0)] * 5
    units, cells = check(index, empty, 3, 5)
    assert units.tolist() == none and len(cells) == 0
    cols = random_works(10, 5, 5, seed=2)
    units, cells = check(index, cols, 10, 0, unit_of=np.full(N_SCRIPT, 7, np.uint32))   # unread
    assert len(units) == 0 and len(cells) == 0
    got = transitions.find_transitions(*cols, 10, N_SCRIPT, unit_map(5), 5, WORDS + 1)
    assert got[0].tolist() == none and len(got[1]) == 0                  # no run is a passage


def test_refusals(index):
    from fandom_search_amd.engine import torch_ready
    cols = random_works(30, 10, 20, seed=9)
    unit_of = unit_map(20)

    def refused(c, n_works=30, unit_of=unit_of, n_units=20, code=abi.FS_E_INVALID,
                n_script=N_SCRIPT, rows=True, **options):
        o = dict(dict(min_words=WORDS, max_gap=0, within=NONE, min_steps=1, min_step_works=1,
                      min_share=0), **options)
        with pytest.raises(_lib.FsError) as e:
            transitions.find_transitions(*c, n_works, n_script, unit_of, n_units, **o)
        assert e.value.code == code
        if rows:
            d_rows, d_map = on_device(c, unit_of)
            torch_ready()
            with pytest.raises(_lib.FsError) as e:
                index.transitions_device(d_rows.data_ptr(), len(c[0]), n_works, d_map.data_ptr(),
                                         n_units, **o)
            assert e.value.code == code
    refused(cols, min_words=0)
    refused(cols, min_steps=0)
    refused(cols, min_step_works=0)
    refused(cols, min_share=101)
    refused(cols, n_works=int(cols[0].max()))              # a work >= n_works
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[40], fan[41] = fan[41] + 1, fan[40]
    assert cols[0][40] == cols[0][41]
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
    units = np.zeros(20, dtype=abi.TRANSITION_UNIT_DTYPE)
    rc = _call(L, cols, 30, unit_of, 20, units, units, 0, n, n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(index, cols, 30, 20)                             # and the same columns are accepted
    ms = (C.c_double * 5)()
    assert L.fs_transitions_times(ms) == abi.FS_OK and min(ms[:3]) > 0 and ms[4] > max(ms[:4])


# ---- the randomised cross-check -------------------------------------------------------------

@pytest.mark.parametrize("seed,n_units", [(1, 1), (2, 7), (3, 40), (4, DENSE), (5, 90)])
def test_random_works_against_the_restatement(index, path, seed, n_units):
    cols = random_works(200, 40, n_units, seed=seed)
    units, cells = check(index, cols, 200, n_units)
    out = np.bincount(cells["a"], weights=cells["steps"], minlength=n_units)
    assert (out == units["steps_out"]).all()               # every cell is kept here
    assert (np.bincount(cells["b"], weights=cells["steps"], minlength=n_units)
            == units["steps_in"]).all()
    recs = list(zip(*(c.tolist() for c in cols)))
    seq = tr.sequence(recs, unit_map(n_units).tolist(), WORDS)
    assert units["starts"].sum() == units["ends"].sum() == len({p["work"] for p in seq})
    assert (cells["advances"] <= cells["steps"]).all() and (cells["works"] <= cells["steps"]).all()
    check(index, cols, 200, n_units, max_gap=1, within=2 * (WORDS + FAN_GAP), min_steps=2,
          min_step_works=2, min_share=10)


# ---- the command ------------------------------------------------------------------------------

def run_both(tmp_path, src, argv):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / reader)
        assert main(["transitions", src, "-o", prefix, "--reader", reader] + argv) == 0
        got[reader] = tuple(open(p, "rb").read() for p in transitions.output_names(src, prefix))
    assert got["device"] == got["python"]
    return got["device"]


@pytest.mark.parametrize("case", mtg.CASES, ids=[c[0] for c in mtg.CASES])
def test_golden_cases_under_both_readers(tmp_path, path, case):
    src = os.path.join(GOLDEN, mtg.INPUT)
    out = run_both(tmp_path, src, mtg.arguments(case))
    with open(src, newline="", encoding="utf-8") as fh:
        want = tr.transitions_csv(fh.read(), **mtg.options(case))
    assert out == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mtg.golden_names(case[0]), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_the_defaults_by_character_and_the_default_prefix(tmp_path):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, mtg.INPUT), src)
    out = run_both(tmp_path, src, [])
    for name, part in zip(mtg.golden_names("default"), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name
    assert main(["transitions", src, "--by", "character", "--min-step-works", "1"]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        want = tr.transitions_csv(fh.read(), "character", min_step_works=1)
    for path_, text in zip(transitions.output_names(src), want):
        with open(path_, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path_
    assert want[0].count("\r\n") > 3 and ",same," in want[0]


def test_an_off_grammar_file_gives_the_python_reader_s_output(tmp_path):
    with open(os.path.join(GOLDEN, mtg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    parts = lines[5].split(b",")
    parts[2] = b'fee"l"in'                       # a quote inside a field: csv.reader takes it
    lines[5] = b",".join(parts)
    src = tmp_path / "m.csv"
    src.write_bytes(b"\r\n".join(lines))
    with MatchFile(str(src)) as mf:
        assert mf.outside and mf.reason & abi.FS_MATCH_BAD_OPEN
    out = run_both(tmp_path, str(src), ["--by", "scene"])
    assert out == tuple(p.encode("utf-8") for p in
                        tr.transitions_csv(src.read_bytes().decode("utf-8"), "scene"))
    with open(os.path.join(GOLDEN, mtg.golden_names("scene")[0]), "rb") as fh:
        assert out[0] == fh.read()               # (a fan word plays no part)
