"""`neighbours` on the GPU: fs_neighbours / fs_neighbours_rows against the restated contract
(tests/neighbours_restated.py), every field of the three record arrays compared for equality,
with the product by MFMA (FS_NEIGHBOURS_MFMA=1) and by the plain kernel (0); active works
around a tile of 64 and around the four column tiles a workgroup's waves take together, script
sizes around a 64-bit word, list lengths 1, all and 32, the column tiles in 1, 2 and more
shares than there are tiles; `pairs` and `quotes` as cross-checks; `ao3.py neighbours` byte for
byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, neighbours, pairs, quotes
from fandom_search_amd.cli import main
from tests import neighbours_restated as nr
from tests.golden import make_neighbours_golden as mng

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fs_neighbours.hip: works of a stripe and of a column tile; column tiles the four waves of a
# workgroup take side by side
TILE = 64
WAVES = 4
N_SCRIPT = 3000          # of the index behind fs_neighbours_rows
DTYPES = (abi.NEIGHBOUR_WORK_DTYPE, abi.NEIGHBOUR_WORD_DTYPE, abi.NEIGHBOUR_DTYPE)


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd import synth
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, n_script, **kw):
    recs = list(zip(*(c.tolist() for c in cols)))
    out = []
    for found, keys, dt in zip(nr.neighbours(recs, n_works, n_script, **kw),
                               (nr.WORK_KEYS, nr.WORD_KEYS, nr.NEIGHBOUR_KEYS), DTYPES):
        a = np.zeros(len(found), dtype=dt)
        for name in keys:
            a[name] = [d[name] for d in found]
        out.append(a)
    return tuple(out)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (dt.names[0], len(a), len(b))
        for name in dt.names:
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def from_spans(spans_of):
    """Records of works given as lists of (first script word, words): a diagonal run per span,
    the fan index jumping between them; an empty list is a work without records."""
    work, fan, orig = [], [], []
    for w, spans in enumerate(spans_of):
        f = 0
        for o0, k in spans:
            work += [w] * k
            fan += range(f, f + k)
            orig += range(o0, o0 + k)
            f += k + 10
    return tuple(np.array(c, dtype=np.uint32) for c in (work, fan, orig))


def fandom(n_active, n_script, seed, m=3):
    """(spans per work, m): one line every active work quotes (its first m words), a pool of
    lines few works quote, every fifth active work a copy of the one before it, the last script
    word covered by two works; between the active works some without a passage (no records, or
    a run one word short)."""
    rng = np.random.default_rng(seed)
    m = min(m, n_script)
    room = n_script - m
    pool = [(int(rng.integers(0, room + 1)), m + int(rng.integers(0, min(m, n_script - m) + 1)))
            for _ in range(max(2, n_active // 3))]
    pool = [(o, min(k, n_script - o)) for o, k in pool]
    out, last = [], None
    for k in range(n_active):
        for _ in range(int(rng.integers(0, 3))):
            out.append([(int(rng.integers(0, room + 1)), m - 1)] if m > 1 and rng.random() < 0.5
                       else [])
        if k % 5 == 4 and last is not None:
            spans = list(last)
        else:
            spans = [(0, m)] + [pool[int(i)] for i in rng.integers(0, len(pool),
                                                                   int(rng.integers(0, 4)))]
            if k in (1, 2):
                spans.append((n_script - m, m))
        out.append(spans)
        last = spans
    out.append([])
    return out, m


def check(monkeypatch, cols, n_works, n_script, index=None, products=("1", "0"), **kw):
    """The host entry point (and, with an index, the device one) under both products against
    the oracle; the last result."""
    want = oracle(cols, n_works, n_script, **kw)
    for mfma in products:
        monkeypatch.setenv("FS_NEIGHBOURS_MFMA", mfma)
        got = neighbours.find_neighbours(*cols, n_works, n_script, **kw)
        assert_equal(got, want)
        if index is not None:
            assert n_script == N_SCRIPT
            assert_equal(on_index(index, cols, n_works, **kw), want)
    monkeypatch.delenv("FS_NEIGHBOURS_MFMA", raising=False)
    return got


def on_index(index, cols, n_works, min_words=6, max_gap=0, weight="rarity", top=10, min_score=1,
             min_similarity=0):
    import torch
    from fandom_search_amd.engine import torch_ready
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name][:len(col)] = col
    d_rows = torch.from_numpy(rows.view(np.uint8)).to("cuda")
    torch_ready()
    works, words, found = index.neighbours_device(
        d_rows.data_ptr(), len(cols[0]), n_works, min_words, max_gap,
        neighbours.weight_code(weight), top, min_score, min_similarity)
    return works, words, found


def test_no_records_and_no_passage(monkeypatch):
    empty = (np.zeros(0, np.uint32),) * 3
    works, words, found = check(monkeypatch, empty, 3, 10)
    assert works.tolist() == [(0, 0, 0, 0, 0, 0, abi.FS_NONE, 0)] * 3
    assert not words["depth"].any() and len(found) == 0
    works, words, found = check(monkeypatch, empty, 0, 0)
    assert len(works) == len(words) == len(found) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32))
    works, words, found = check(monkeypatch, one, 3, 10, min_words=2)   # a record, no passage
    assert not works["covered"].any() and not words["depth"].any()
    works, words, found = check(monkeypatch, one, 3, 10, min_words=1)   # N = 1
    assert works[1].tolist() == (1, 1, 0, 0, 0, 0, abi.FS_NONE, 0) and len(found) == 0
    assert words[9].tolist() == (1, 1)


@pytest.mark.parametrize("n_active", [2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE,
                                      2 * TILE + 1, WAVES * TILE - 1, WAVES * TILE,
                                      WAVES * TILE + 1])
def test_active_works_around_a_tile_and_a_workgroup(monkeypatch, n_active):
    n_script = 300
    spans_of, m = fandom(n_active, n_script, seed=n_active)
    cols = from_spans(spans_of)
    assert len(spans_of) > n_active + 1
    works, words, found = check(monkeypatch, cols, len(spans_of), n_script, min_words=m)
    assert (works["covered"] > 0).sum() == n_active
    # the weights span 1 .. N.bit_length(): the line everybody quotes, a line of one work
    if n_active >= TILE - 1:
        assert words["weight"].min() == 0 and words["weight"][0] == 1
        assert words["weight"].max() == n_active.bit_length()
        assert len(found) > n_active and (found["ppm"] == 1000000).any()    # the copies
    # every pair is a candidate (the shared line), only `top` are listed
    active = works["covered"] > 0
    assert (works["candidates"][active] == n_active - 1).all()
    assert (works["listed"][active] == min(10, n_active - 1)).all()
    assert works["listed_by"].sum() == works["listed"].sum() == len(found)


@pytest.mark.parametrize("n_script", [1, 63, 64, 65, 32 * 64 + 1])
def test_script_sizes_around_a_word(monkeypatch, n_script):
    spans_of, m = fandom(70, n_script, seed=n_script)
    cols = from_spans(spans_of)
    works, words, found = check(monkeypatch, cols, len(spans_of), n_script, min_words=m)
    assert words["depth"][n_script - 1] >= 2 and len(found) >= 70
    if n_script > 1:
        check(monkeypatch, cols, len(spans_of), n_script, min_words=m, max_gap=1, min_score=2,
              weight="flat")


@pytest.mark.parametrize("top", [1, 32])
@pytest.mark.parametrize("n_active", [20, 33, 150])
def test_list_lengths(monkeypatch, n_active, top):
    """top 32 with 20 and 33 active works: at least N - 1, every candidate listed."""
    spans_of, m = fandom(n_active, 200, seed=100 + n_active)
    cols = from_spans(spans_of)
    works, words, found = check(monkeypatch, cols, len(spans_of), 200, min_words=m, top=top)
    active = works["covered"] > 0
    assert (works["listed"][active] == min(top, n_active - 1)).all()
    if top == 32 and n_active <= 33:
        assert (found["back_rank"] != abi.FS_NONE).all()              # everybody lists everybody
        assert (works["mutual"][active] == n_active - 1).all()


@pytest.mark.parametrize("split", ["1", "2", "3", "40"])
def test_column_tiles_in_shares(monkeypatch, split):
    """Five column tiles in 1, 2 and 3 shares (the last share of three holds one tile: three of
    its waves have none) and in more shares than tiles."""
    n_active = 4 * TILE + 9
    spans_of, m = fandom(n_active, 260, seed=7)
    cols = from_spans(spans_of)
    monkeypatch.setenv("FS_NEIGHBOURS_SPLIT", split)
    check(monkeypatch, cols, len(spans_of), 260, min_words=m, top=7, min_similarity=20)
    monkeypatch.delenv("FS_NEIGHBOURS_SPLIT", raising=False)


def test_thresholds_and_weights(monkeypatch):
    spans_of, m = fandom(90, 150, seed=3)
    cols = from_spans(spans_of)
    base = check(monkeypatch, cols, len(spans_of), 150, min_words=m)
    for kw in (dict(min_score=7), dict(min_similarity=40), dict(min_similarity=100),
               dict(weight="flat", top=3), dict(weight="flat", min_score=4, min_similarity=34)):
        works, words, found = check(monkeypatch, cols, len(spans_of), 150, min_words=m, **kw)
        assert (works["candidates"] <= base[0]["candidates"]).all()
        assert (works["own"] == base[0]["own"]).all() or kw.get("weight") == "flat"
    assert (found["ppm"] >= 340000).all() and len(found) > 0


def test_both_entry_points_over_an_index(monkeypatch, index):
    spans_of, m = fandom(2 * TILE + 5, N_SCRIPT, seed=11)
    cols = from_spans(spans_of)
    check(monkeypatch, cols, len(spans_of), N_SCRIPT, index=index, min_words=m)
    check(monkeypatch, cols, len(spans_of), N_SCRIPT, index=index, min_words=m, max_gap=1,
          weight="flat", top=32, min_score=2, min_similarity=10)
    empty = (np.zeros(0, np.uint32),) * 3
    check(monkeypatch, empty, 4, N_SCRIPT, index=index)


def test_the_run_around_the_rarest_word_across_word_boundaries(monkeypatch):
    n_script = 200
    spans_of = [[(0, 8), (60, 11)],               # 60..70, across the bit 63 | 64
                [(0, 8), (50, 30)],
                [(0, 8), (192, 8)],               # up to the last script word
                [(0, 8), (120, 80)],
                [(0, 200)],
                [(0, 8)], [(0, 8)], [(0, 8)], [(0, 8)]]
    works, words, found = check(monkeypatch, from_spans(spans_of), 9, n_script, min_words=2)
    by = {(int(p["a"]), int(p["b"])): p for p in found}
    assert (by[0, 1]["rarest"], by[0, 1]["run_first"], by[0, 1]["run_words"]) == (60, 60, 11)
    assert (by[2, 3]["run_first"], by[2, 3]["run_words"]) == (192, 8)
    assert (by[3, 4]["run_first"], by[3, 4]["run_words"]) == (120, 80)   # over two boundaries
    assert (by[5, 6]["rarest"], by[5, 6]["run_first"], by[5, 6]["run_words"]) == (0, 0, 8)


def test_capacity_too_small_by_one_exact_and_zero(monkeypatch):
    spans_of, m = fandom(100, 300, seed=8)
    cols = [np.ascontiguousarray(c) for c in from_spans(spans_of)]
    n_works = len(spans_of)
    want = oracle(cols, n_works, 300, min_words=m, top=4)
    k = len(want[2])
    assert k == 400
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.NEIGHBOUR_WORK_DTYPE)
    words = np.zeros(300, dtype=abi.NEIGHBOUR_WORD_DTYPE)
    found = np.zeros(k, dtype=abi.NEIGHBOUR_DTYPE)
    n = C.c_uint64(0)

    def call(cap):
        return L.fs_neighbours(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                               abi.ptr(cols[2], C.c_uint32), len(cols[0]), n_works, 300, m, 0,
                               0, 4, 1, 0, works.ctypes.data_as(C.c_void_p),
                               words.ctypes.data_as(C.c_void_p),
                               found.ctypes.data_as(C.c_void_p) if cap else None, cap,
                               C.byref(n))
    for cap in (k - 1, 0):
        works[:] = 0
        words[:] = 0
        assert call(cap) == abi.FS_E_CAPACITY and n.value == k
        assert_equal((works, words, want[2]), want)        # works and words are complete
        assert not found["b"].any()                        # the listed pairs untouched
    assert call(k) == abi.FS_OK and n.value == k
    assert_equal((works, words, found), want)


def test_refusals():
    spans_of, m = fandom(10, 100, seed=5)
    cols = from_spans(spans_of)
    n_works = len(spans_of)

    def refused(c=cols, n_works=n_works, n_script=100, code=abi.FS_E_INVALID, **kw):
        with pytest.raises(_lib.FsError) as e:
            neighbours.find_neighbours(*c, n_works, n_script, **kw)
        assert e.value.code == code
    refused(min_words=0)
    refused(min_score=0)
    refused(top=0)
    refused(top=33)
    refused(min_similarity=101)
    refused(n_works=n_works - 3)                           # a work >= n_works
    refused(n_script=int(cols[2].max()))                   # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[0], fan[1] = fan[1] + 1, fan[0]
    refused((cols[0], fan, cols[2]))
    refused(n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED)
    # 16 385 works of one record each over 2^19 script words: a matrix above 1 GiB by itself
    many = abi.FS_NEIGHBOURS_MAX_BYTES // ((1 << 19) // 8) + 1
    one = (np.arange(many, dtype=np.uint32), np.zeros(many, np.uint32),
           np.arange(many, dtype=np.uint32) % 5000)
    refused(one, n_works=many, n_script=1 << 19, min_words=1, code=abi.FS_E_UNSUPPORTED)


def test_flat_neighbours_are_the_partners_of_pairs(monkeypatch):
    """Under --weight flat --min-similarity 0 and a list that holds every candidate, a work's
    candidates are its partners in `pairs` at --min-shared = --min-score, SCORE is the pair's
    shared words, and DEPTH is the depth `quotes` gives the word."""
    spans_of, m = fandom(30, 120, seed=21)
    cols = from_spans(spans_of)
    n_works = len(spans_of)
    for s in (1, 4):
        works, words, found = check(monkeypatch, cols, n_works, 120, min_words=m, weight="flat",
                                    top=32, min_score=s)
        pworks, pfound = pairs.find_pairs(*cols, n_works, 120, m, 0, s)
        assert (works["covered"] == pworks["covered"]).all()
        assert (works["candidates"] == pworks["partners"]).all()
        assert (works["listed"] == pworks["partners"]).all()
        shared = {}
        for p in pfound:
            shared[int(p["a"]), int(p["b"])] = shared[int(p["b"]), int(p["a"])] = int(p["shared"])
        assert {(int(p["a"]), int(p["b"])): int(p["score"]) for p in found} == shared
        assert (found["score"] == found["shared"]).all()
    comb = np.zeros(len(cols[0]), dtype=np.float64)
    qwords, _ = quotes.find_quotes(*cols, comb, n_works, 120, m, 0, 1)
    assert (words["depth"] == qwords["n_passage_works"]).all() and words["depth"].any()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,options,kw", mng.CASES)
def test_command_on_the_golden_cases(tmp_path, case, options, kw, reader):
    src = os.path.join(GOLDEN, mng.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["neighbours", src, "-o", prefix, "--reader", reader] + options) == 0
    got = tuple(open(p, "rb").read() for p in neighbours.output_names(src, prefix))
    with open(src, newline="", encoding="utf-8") as fh:
        want = nr.neighbours_csv(fh.read(), **kw)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mng.golden_names(case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name
