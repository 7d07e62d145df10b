"""`tree` on the GPU: fs_tree / fs_tree_rows against the restated contract
(tests/tree_restated.py), every field of every work, merge and level compared for equality;
numbers of works, of column tiles and of script words around every size the kernels treat
differently; ties on every edge; paths that take a known number of rounds; cuts of the tree
against `clusters` and `pairs`; `ao3.py tree` byte for byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, clusters, pairs, tree
from fandom_search_amd.cli import main
from tests import tree_restated as tr
from tests.golden import make_tree_golden as mtg
from tests.test_gpu_clusters import shuffled
from tests.test_gpu_pairs import CHUNK, K_SLICE, TILE, from_spans, interleaved, records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
DTYPES = (abi.TREE_WORK_DTYPE, abi.TREE_MERGE_DTYPE, abi.TREE_LEVEL_DTYPE)
N_SCRIPT = 300


def oracle(cols, n_works, n_script, m, g, measure, s, level):
    recs = list(zip(*(c.tolist() for c in cols)))
    out = []
    for found, keys, dt in zip(tr.tree(recs, n_works, n_script, m, g, measure, s, level),
                               (tr.WORK_KEYS, tr.MERGE_KEYS, tr.LEVEL_KEYS), DTYPES):
        a = np.zeros(len(found), dtype=dt)
        for name in keys:
            a[name] = [d[name] for d in found]
        out.append(a)
    return tuple(out)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (dt.names[0], len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def check(cols, n_works, n_script, m=6, g=0, measure="jaccard", s=6, level=0):
    got = tree.find_tree(*cols, n_works, n_script, m, g, measure, s, level)
    assert_equal(got, oracle(cols, n_works, n_script, m, g, measure, s, level))
    return got


def times():
    ms = (C.c_double * len(abi.TREE_MS_NAMES))()
    assert _lib.load().fs_tree_times(ms) == abi.FS_OK
    return dict(zip(abi.TREE_MS_NAMES, ms))


# ---- sizes ------------------------------------------------------------------------------

def test_no_records_and_one_record():
    empty = (np.zeros(0, np.uint32),) * 3
    none = (0, NONE, 0, 0, NONE, 0, NONE, NONE)
    works, merges, levels = check(empty, 3, 10)
    assert works.tolist() == [none] * 3 and len(merges) == 0 and len(levels) == 0
    works, merges, levels = check(empty, 0, 0)
    assert len(works) == 0 and len(merges) == 0 and len(levels) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32))
    works, merges, levels = check(one, 3, 10, m=1, s=1)
    assert works.tolist() == [none, (1, 0, 1, 0, NONE, 0, NONE, 0), none]
    assert len(merges) == 0 and len(levels) == 0 and times()["rounds"] == 0
    works, merges, levels = check(one, 3, 10, m=2, s=1)
    assert works.tolist() == [none] * 3


@pytest.mark.parametrize("n_active", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_active_works_around_the_tile(n_active):
    n_script = 300
    spans_of = interleaved(n_active, lambda k, rng: [
        (int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))
        for _ in range(int(rng.integers(1, 4)))], seed=n_active)
    cols = from_spans(spans_of)
    assert len(spans_of) > n_active + 1
    works, merges, levels = check(cols, len(spans_of), n_script, m=3, s=1)
    assert (works["covered"] > 0).sum() == n_active
    assert sorted(works["leaf"][works["covered"] > 0].tolist()) == list(range(n_active))
    check(cols, len(spans_of), n_script, m=3, measure="shared", s=4, level=5)


@pytest.mark.parametrize("tiles", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_column_tiles_around_a_chunk(tiles):
    n_active = (tiles - 1) * TILE + 5
    rng = np.random.default_rng(tiles)
    spans_of = [[(int(rng.integers(0, 59)), int(rng.integers(1, 3)))] for _ in range(n_active)]
    cols = from_spans(spans_of)
    works, merges, levels = check(cols, n_active, 60, m=1, s=1)
    # an edge across the chunks: the last work's first edge goes to a work of the first tiles
    assert works["best"][n_active - 1] < (tiles - 2) * TILE
    assert len(merges) > n_active - 60
    check(cols, n_active, 60, m=1, measure="shared", s=2)


@pytest.mark.parametrize("n_script", [1, 63, 64, 65, 64 * K_SLICE - 1, 64 * K_SLICE,
                                      64 * K_SLICE + 1])
def test_script_sizes_around_a_word_and_a_slice(n_script):
    sizes = np.random.default_rng(n_script).integers(0, 60, size=70)
    sizes[[3, 66]] = 5
    cols = records(sizes, n_script, seed=n_script)
    # the last script word, the last bit of the last 64-bit word, shared by two works
    for w in (3, 66):
        at = int(np.nonzero(cols[0] == w)[0][0])
        cols[2][at] = n_script - 1
    works, merges, levels = check(cols, 70, n_script, m=1, s=1)
    assert works["tree"][3] == works["tree"][66] != NONE
    check(cols, 70, n_script, m=1, measure="shared", s=1)
    if n_script > 1:
        check(cols, 70, n_script, m=3, g=1, s=2, level=200000)


# ---- ties -------------------------------------------------------------------------------

@pytest.mark.parametrize("measure,level", [("jaccard", 1000000), ("shared", 12)])
def test_129_identical_works(measure, level):
    spans_of = [[(70, 9), (120, 3)] for _ in range(129)]
    works, merges, levels = check(from_spans(spans_of), 129, 300, m=3, measure=measure, s=12)
    k = np.arange(1, 129)
    assert (merges["a"] == 0).all() and (merges["b"] == k).all()
    assert (merges["level"] == level).all() and (merges["shared"] == 12).all()
    assert merges["left"].tolist() == [NONE] + list(range(127))
    assert (merges["right"] == NONE).all() and (merges["right_works"] == 1).all()
    assert (merges["left_works"] == k).all() and (merges["works"] == k + 1).all()
    assert (merges["run_first"] == 70).all() and (merges["run_words"] == 9).all()
    assert works["leaf"].tolist() == list(range(129))
    assert works["best"].tolist() == [1] + [0] * 128
    assert levels.tolist() == [(level, 128, 0, 1, 129, 129, 0, 0)]
    assert times()["rounds"] == 1
    # the same works between works without a passage
    mixed = interleaved(129, lambda k, rng: [(70, 9), (120, 3)], seed=3)
    works, merges, levels = check(from_spans(mixed), len(mixed), 300, m=3, measure=measure, s=12)
    assert len(merges) == 128 and len(set(merges["a"].tolist())) == 1


@pytest.mark.parametrize("measure", ["jaccard", "shared"])
def test_three_groups_in_three_tiles_with_every_triangle_tied(measure):
    # five works on 0..9 + 10..14, five on 0..9 + 20..24, five on 0..9 + 30..34, at the start of
    # three tiles; every pair across two groups shares 10 of 20.  The other works of the tiles
    # quote three words of their own each.
    spans_of = [[(100 + 3 * k, 3)] for k in range(2 * TILE + 5)]
    for g in range(3):
        for k in range(5):
            spans_of[g * TILE + k] = [(0, 10), (10 + 10 * g, 5)]
    n = len(spans_of)
    works, merges, levels = check(from_spans(spans_of), n, 100 + 3 * n, m=3, measure=measure, s=3)
    assert len(merges) == 14 and len(levels) == 2
    assert merges["a"][:12].tolist() == [0] * 4 + [TILE] * 4 + [2 * TILE] * 4
    assert merges[12:][["a", "b"]].tolist() == [(0, TILE), (0, 2 * TILE)]
    assert merges["left_works"][12:].tolist() == [5, 10]
    order = shuffled(spans_of, seed=8)
    check(from_spans(order), n, 100 + 3 * n, m=3, measure=measure, s=3)


# ---- rounds -----------------------------------------------------------------------------

def path(overlaps, words):
    """Works of `words` script words each, work k + 1 starting overlaps[k] words before the end
    of work k."""
    spans_of, at = [[(0, words)]], 0
    for ov in overlaps:
        at += words - ov
        spans_of.append([(at, words)])
    return spans_of, at + words


@pytest.mark.parametrize("seed", [None, 5])
def test_a_path_of_64_works_takes_six_rounds(seed):
    # works k and k + 1 overlap by 12 - v words, v the trailing zero bits of k + 1: every round
    # joins the families in twos
    overlaps = [12 - ((k + 1) & -(k + 1)).bit_length() + 1 for k in range(63)]
    assert overlaps[:8] == [12, 11, 12, 10, 12, 11, 12, 9] and min(overlaps) == 7
    spans_of, n_script = path(overlaps, 30)
    if seed is not None:
        spans_of = shuffled(spans_of, seed)
    works, merges, levels = check(from_spans(spans_of), 64, n_script, m=3, measure="shared", s=1)
    assert len(merges) == 63 and times()["rounds"] == 6
    assert merges["level"].tolist() == sorted(overlaps, reverse=True)
    assert (works["tree_works"] == 64).all() and merges["works"][-1] == 64


def test_a_path_of_200_works_hooked_in_one_round():
    # the overlaps grow along the path: every work chooses its successor, the last one its
    # predecessor, and one round hooks a chain of 199
    overlaps = list(range(1, 200))
    spans_of, n_script = path(overlaps, 400)
    works, merges, levels = check(from_spans(spans_of), 200, n_script, m=3, measure="shared",
                                  s=1)
    assert len(merges) == 199 and times()["rounds"] == 1
    assert merges["level"].tolist() == overlaps[::-1]
    assert merges[["a", "b"]].tolist() == [(k, k + 1) for k in range(198, -1, -1)]
    assert works["leaf"].tolist() == list(range(200))
    order = shuffled(spans_of, seed=1, first=57)
    works, merges, levels = check(from_spans(order), 200, n_script, m=3, measure="shared", s=1)
    assert len(merges) == 199 and times()["rounds"] == 1


# ---- forest -----------------------------------------------------------------------------

def test_disjoint_groups_and_works_below_min_shared():
    # four groups of works on lines of their own; work 12 shares five words with the first
    # group, one fewer than --min-shared; work 13 shares nothing
    spans_of = [[(40 * (k % 4), 8 + k // 4)] for k in range(12)] + [[(3, 5), (200, 4)]] + \
        [[(300, 9)]]
    works, merges, levels = check(from_spans(spans_of), 14, 320, m=3)
    assert len(merges) == 8 and works["edges"][12] == 0 and works["edges"][13] == 0
    assert sorted(works["tree_works"].tolist()) == [1, 1] + [3] * 12
    assert len(set(works["tree"].tolist())) == 6
    works, merges, levels = check(from_spans(spans_of), 14, 320, m=3, s=5)
    assert works["edges"][12] == 1 and len(merges) == 9


@pytest.mark.parametrize("measure", ["jaccard", "shared"])
def test_min_level_at_a_level_and_one_above(measure):
    sizes = np.random.default_rng(21).integers(0, 60, size=90)
    cols = records(sizes, 200, seed=21)
    works, merges, levels = check(cols, 90, 200, m=3, measure=measure, s=2)
    assert len(levels) > 4
    at = int(levels["level"][len(levels) // 2])
    kept = check(cols, 90, 200, m=3, measure=measure, s=2, level=at)
    assert kept[2]["level"].min() == at
    # the merges at or above the bar are those of the whole tree (the ranks of the trees, which
    # the later merges decide, aside), and so are the level rows
    same = [n for n in abi.TREE_MERGE_DTYPE.names if n != "tree"]
    assert (kept[1][same] == merges[merges["level"] >= at][same]).all()
    assert (kept[2] == levels[levels["level"] >= at]).all()
    dropped = check(cols, 90, 200, m=3, measure=measure, s=2, level=at + 1)
    assert dropped[2]["level"].min() > at
    assert len(dropped[1]) == len(kept[1]) - int(levels["merges"][len(levels) // 2])


# ---- cuts against code that exists ------------------------------------------------------

@pytest.fixture(scope="module")
def random_input():
    sizes = np.random.default_rng(12).integers(3, 60, size=300)
    return records(sizes, N_SCRIPT, seed=12)


@pytest.fixture(scope="module")
def random_tree(random_input):
    return check(random_input, 300, N_SCRIPT, m=3, s=2)


@pytest.mark.parametrize("j", [0, 30, 50, 100])
def test_a_cut_of_the_tree_is_the_partition_of_clusters(random_input, random_tree, j):
    works, merges, levels = random_tree
    assert (works["covered"] > 0).sum() > 250
    cworks, found = clusters.find_clusters(*random_input, 300, N_SCRIPT, 3, 0, 2, j, 2, 50)
    root = np.where(works["covered"] > 0, np.arange(300), NONE).astype(np.int64)

    def find(w):
        while root[w] != w:
            w = root[w]
        return w
    for m in merges[merges["level"] >= j * 10000]:
        a, b = find(int(m["a"])), find(int(m["b"]))
        assert a != b
        root[max(a, b)] = min(a, b)
    cut = [find(w) if works["covered"][w] else NONE for w in range(300)]
    assert cut == cworks["root"].tolist()
    above = levels[levels["level"] >= j * 10000]
    if len(above) == 0:
        assert len(found) == 0
        return
    assert above[-1]["families"] == len(found)
    assert above[-1]["largest"] == found["n_works"].max()
    assert above[-1]["singles"] == (cworks["size"] == 1).sum()


def test_the_first_edge_under_shared_is_the_best_partner_of_pairs(random_input):
    works, merges, levels = check(random_input, 300, N_SCRIPT, m=3, measure="shared", s=2)
    pworks, _ = pairs.find_pairs(*random_input, 300, N_SCRIPT, 3, 0, 2)
    assert (works["best"] == pworks["best"]).all()
    assert (works["joined_level"] == pworks["best_shared"]).all()
    assert (works["covered"] == pworks["covered"]).all()


# ---- calls ------------------------------------------------------------------------------

def _call(L, cols, n_works, n_script, params, works, merges, cap_m, n_m, levels, cap_l, n_l,
          n_rows=None):
    m, measure, s, level = params
    return L.fs_tree(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                     abi.ptr(cols[2], C.c_uint32), len(cols[0]) if n_rows is None else n_rows,
                     n_works, n_script, m, 0, measure, s, level,
                     works.ctypes.data_as(C.c_void_p),
                     merges.ctypes.data_as(C.c_void_p) if cap_m else None, cap_m, C.byref(n_m),
                     levels.ctypes.data_as(C.c_void_p) if cap_l else None, cap_l, C.byref(n_l))


def test_capacity_too_small_by_one_exact_and_zero(random_input, random_tree):
    cols = [np.ascontiguousarray(c) for c in random_input]
    want = random_tree
    km, kl = len(want[1]), len(want[2])
    assert km > 100 and kl > 10
    L = _lib.load()
    works = np.zeros(300, dtype=abi.TREE_WORK_DTYPE)
    merges = np.zeros(km, dtype=abi.TREE_MERGE_DTYPE)
    levels = np.zeros(kl, dtype=abi.TREE_LEVEL_DTYPE)
    n_m, n_l = C.c_uint64(0), C.c_uint64(0)
    params = (3, abi.FS_TREE_JACCARD, 2, 0)
    for cap_m, cap_l in ((km - 1, kl), (0, kl), (km, kl - 1), (km, 0), (0, 0)):
        works[:] = 0
        rc = _call(L, cols, 300, N_SCRIPT, params, works, merges, cap_m, n_m, levels, cap_l, n_l)
        assert rc == abi.FS_E_CAPACITY and (n_m.value, n_l.value) == (km, kl)
        assert_equal((works,), want[:1])                   # the works are complete
        assert not merges["works"].any() and not levels["merges"].any()      # the rest untouched
    assert _call(L, cols, 300, N_SCRIPT, params, works, merges, km, n_m, levels, kl,
                 n_l) == abi.FS_OK and (n_m.value, n_l.value) == (km, kl)
    assert_equal((works, merges, levels), want)
    t = times()
    assert t["rounds"] >= 2 and all(t[k] > 0 for k in abi.TREE_MS_NAMES)
    assert t["total"] >= t["best"] + t["replay"]


def test_refusals():
    """include/fandom_search.h.  The accepted side of FS_TREE_MAX_BYTES, tables of 1 GiB, is not
    tested: only that one work more is refused.  A work counts nk * 8 + FS_TREE_ROW_BYTES bytes,
    so a work is the smallest step above the limit."""
    cols = records([300, 500, 200], 1000, seed=9)

    def refused(c, n_works=3, n_script=1000, m=6, measure="jaccard", s=6, level=0,
                code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            tree.find_tree(*c, n_works, n_script, m, 0, measure, s, level)
        assert e.value.code == code
    refused(cols, m=0)
    refused(cols, s=0)
    refused(cols, level=1000001)
    refused(cols, n_works=2)                               # a work >= n_works
    refused(cols, n_script=int(cols[2].max()))             # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))
    refused(cols, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED)
    L = _lib.load()
    n_m, n_l = C.c_uint64(0), C.c_uint64(0)
    works = np.zeros(3, dtype=abi.TREE_WORK_DTYPE)
    rc = _call(L, cols, 3, 1000, (6, 0, 6, 0), works, works, 0, n_m, works, 0, n_l,
               n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    rc = _call(L, cols, 3, 1000, (6, 2, 6, 0), works, works, 0, n_m, works, 0, n_l)
    assert rc == abi.FS_E_INVALID                          # a measure that is none
    check(cols, 3, 1000)                                   # and the same columns are accepted
    check(cols, 3, 1000, measure="shared", level=1000001)  # a level of shared words may be large
    # works of one record each, a passage at --min-words 1, over 2^18 script words: a row of
    # 4 096 words of 8 bytes and 60 bytes of tables per work, one work above FS_TREE_MAX_BYTES
    nk = (1 << 18) // 64
    per = nk * 8 + abi.FS_TREE_ROW_BYTES
    many = abi.FS_TREE_MAX_BYTES // per + 1
    assert (many - 1) * per <= abi.FS_TREE_MAX_BYTES < many * per
    one = (np.arange(many, dtype=np.uint32), np.zeros(many, np.uint32),
           np.arange(many, dtype=np.uint32) % 5000)
    refused(one, n_works=many, n_script=1 << 18, m=1, s=1, code=abi.FS_E_UNSUPPORTED)
    # the same columns, accepted over a smaller script: a script word is a tree
    works, merges, levels = tree.find_tree(*one, many, 5000, 1, 0, "jaccard", 1, 0)
    assert (works["covered"] == 1).all() and len(merges) == many - 5000
    assert levels.tolist() == [(1000000, many - 5000, 0, 5000, many // 5000 + 1, many, 0, 0)]
    assert (merges["a"] == merges["b"] % 5000).all() and (merges["first_work"] == merges["a"]).all()
    assert sorted(set(works["tree_works"].tolist())) == [many // 5000, many // 5000 + 1]


# ---- device rows ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd import synth
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def test_device_rows(index, random_input, random_tree):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols = random_input
    rows = np.zeros(len(cols[0]), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name] = col
    d_rows = torch.from_numpy(rows.view(np.uint8)).to("cuda")
    torch_ready()
    got = index.tree_device(d_rows.data_ptr(), len(rows), 300, 3, 0, "jaccard", 2, 0)
    assert_equal(got, random_tree)
    for measure, g, s, level in (("shared", 1, 3, 4), ("jaccard", 0, 6, 250000)):
        dev = index.tree_device(d_rows.data_ptr(), len(rows), 300, 3, g, measure, s, level)
        assert_equal(dev, oracle(cols, 300, N_SCRIPT, 3, g, measure, s, level))
    # the caller's own device buffers, each too small by one first
    works, merges, levels = random_tree
    km, kl = len(merges), len(levels)
    d_works = torch.zeros(300 * 32, dtype=torch.uint8, device="cuda")
    d_merges = torch.zeros(km * 64, dtype=torch.uint8, device="cuda")
    d_levels = torch.zeros(kl * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_works.data_ptr(), d_merges.data_ptr(), d_levels.data_ptr())
    for caps in ((km - 1, kl), (km, kl - 1)):
        with pytest.raises(_lib.FsError) as e:
            index.tree_device(d_rows.data_ptr(), len(rows), 300, 3, 0, "jaccard", 2, 0,
                              out_ptrs=ptrs, caps=caps)
        assert e.value.code == abi.FS_E_CAPACITY and e.value.required == (km, kl)
        assert (d_works.cpu().numpy().view(abi.TREE_WORK_DTYPE) == works).all()
        assert not d_merges.cpu().numpy().any() and not d_levels.cpu().numpy().any()
    assert index.tree_device(d_rows.data_ptr(), len(rows), 300, 3, 0, "jaccard", 2, 0,
                             out_ptrs=ptrs, caps=(km, kl)) == (km, kl)
    assert (d_merges.cpu().numpy().view(abi.TREE_MERGE_DTYPE) == merges).all()
    assert (d_levels.cpu().numpy().view(abi.TREE_LEVEL_DTYPE) == levels).all()
    # no records: works without coverage on the device
    assert index.tree_device(d_rows.data_ptr(), 0, 300, 3, out_ptrs=ptrs, caps=(km, kl)) == (0, 0)
    none = d_works.cpu().numpy().view(abi.TREE_WORK_DTYPE)
    assert (none["tree"] == NONE).all() and not none["covered"].any()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,options,kw", mtg.CASES)
def test_command_on_the_golden_input(tmp_path, case, options, kw, reader):
    src = os.path.join(GOLDEN, mtg.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["tree", src, "-o", prefix, "--reader", reader] + options) == 0
    got = tuple(open(f, "rb").read() for f in tree.output_names(src, prefix))
    with open(src, newline="", encoding="utf-8") as fh:
        want = tr.tree_csv(fh.read(), **kw)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mtg.golden_names(case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name
