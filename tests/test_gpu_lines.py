"""`lines` on the GPU: fs_lines and fs_lines_rows against the restated contract
(tests/lines_restated.py), every field of every line, work and cell compared for equality, the
reserved words too; line lengths, line positions inside a 64-bit coverage word, numbers of
active works and chunks of lines around every size the kernels treat differently; the counts of
fs_companions and fs_pairs on the same records; `ao3.py lines` byte for byte against the
committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, companions, lines, pairs, synth
from fandom_search_amd.cli import main
from tests import lines_restated as lr
from tests.golden import make_lines_golden as mlg
from tests.test_gpu_pairs import from_spans, interleaved

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
N_SCRIPT = 3000          # of the index behind fs_lines_rows; every case uses it
DTYPES = (abi.LINE_DTYPE, abi.LINE_WORK_DTYPE, abi.LINE_CELL_DTYPE)
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 200)


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, line_first, m, g, most):
    recs = list(zip(*(c.tolist() for c in cols)))
    parts = lr.lines(recs, n_works, N_SCRIPT, list(line_first), m, g, most)
    out = []
    for part, keys, dt in zip(parts, (lr.LINE_KEYS, lr.WORK_KEYS, lr.CELL_KEYS), DTYPES):
        a = np.zeros(len(part), dtype=dt)                  # (the reserved words: 0)
        for name in keys:
            a[name] = [d[name] for d in part]
        out.append(a)
    return tuple(out)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved words, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def on_device(cols, line_first):
    """(rows tensor, line table tensor) in HBM."""
    import torch
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name][:len(col)] = col
    return (torch.from_numpy(rows.view(np.uint8)).to("cuda"),
            torch.from_numpy(np.ascontiguousarray(line_first, dtype=np.uint32)).to("cuda"))


def check(index, cols, n_works, line_first, m=3, g=0, most=50, whole=True, partial=True,
          runs2=False):
    """Both entry points against the oracle, which must hold a whole cell, a partial one and one
    in two runs where the case is meant to; the oracle's result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, n_works, line_first, m, g, most)
    size = np.diff(np.asarray(line_first, dtype=np.int64))[want[2]["line"]]
    assert not whole or (want[2]["covered"] == size).any()
    assert not partial or (want[2]["covered"] < size).any()
    assert not runs2 or (want[2]["runs"] >= 2).any()
    got = lines.find_lines(*cols, n_works, N_SCRIPT, line_first, m, g, most)
    assert_equal(got, want)
    d_rows, d_table = on_device(cols, line_first)
    torch_ready()
    dev = index.lines_device(d_rows.data_ptr(), len(cols[0]), n_works, d_table.data_ptr(),
                             len(line_first) - 1, m, g, most)
    assert_equal(dev, want)
    return want


def random_table(seed, mean=12):
    """A line table over the script: lines of 1 .. 2 * mean - 1 words and a few monologues."""
    rng = np.random.default_rng(seed)
    at, first = 0, []
    while at < N_SCRIPT:
        first.append(at)
        at += int(rng.integers(150, 301)) if rng.random() < 0.01 else int(rng.integers(1, 2 * mean))
    return first + [N_SCRIPT]


def random_works(n_active, seed, lo=3, hi=40, most=3):
    """Active works of 1 .. most random spans and one stretch of seven words quoted without its
    middle word (two runs where it lies in one line), between works without a passage."""
    def spans(k, rng):
        at = int(rng.integers(0, N_SCRIPT - 7))
        return [(int(rng.integers(0, N_SCRIPT - hi)), int(rng.integers(lo, hi + 1)))
                for _ in range(int(rng.integers(1, most + 1)))] + [(at, 3), (at + 4, 3)]
    spans_of = interleaved(n_active, spans, seed=seed)
    return from_spans(spans_of), len(spans_of)


# ---- line lengths and where a line starts in a coverage word ---------------------------------

def placed_table(bit):
    """(line table, the lines of LENGTHS): each of them starts at bit `bit` of a 64-bit word of
    the coverage, filler lines between them."""
    first, special, at = [], [], 0
    for n in LENGTHS:
        start = at + (bit - at) % 64
        if start > at:
            first.append(at)                               # a filler line
        special.append(len(first))
        first.append(start)
        at = start + n
    return first + [at, N_SCRIPT], special


@pytest.mark.parametrize("bit", [0, 1, 63])
def test_line_lengths_at_the_start_inside_and_at_the_end_of_a_coverage_word(index, bit):
    table, special = placed_table(bit)
    spans_of = []
    for l in special:
        a, n = table[l], table[l + 1] - table[l]
        spans_of.append([(a, n)])                                      # whole
        spans_of.append([(a + k, 1) for k in range(0, n, 2)])          # every other word
        if n >= 3:
            spans_of.append([(a, n // 2), (a + n // 2 + 1, n - n // 2 - 1)])   # but one word
            spans_of.append([(a + 1, n - 2)])                          # neither end
        if n >= 2:
            spans_of.append([(a, 1)])                                  # the first word
            spans_of.append([(b, 1) for b in (a + n - 1,)])            # the last word
        spans_of.append([(max(a - 1, 0), 2 if a else 1)])              # from the line before
        spans_of.append([(a + n - 1, 2)])                              # into the line behind
    spans_of.append([(0, table[-2])])                                  # every special line
    cols = from_spans(spans_of)
    want = check(index, cols, len(spans_of), table, m=1, runs2=True)
    cells = want[2]
    for l in special:
        n = table[l + 1] - table[l]
        mine = cells[cells["line"] == l]
        assert mine["covered"].max() == n and mine["runs"].max() == (n + 1) // 2
        assert want[0]["head_works"][l] >= 3 and want[0]["tail_works"][l] >= 3
    # and under a random cover with passages of three and more words
    cols, n_works = random_works(40, seed=bit, hi=250, most=5)
    check(index, cols, n_works, table, m=3, runs2=True)


def test_sixty_four_one_word_lines_in_one_coverage_word(index):
    table = [0] + list(range(64, 129)) + [N_SCRIPT]            # lines 1 .. 64: words 64 .. 127
    spans_of = interleaved(30, lambda k, rng: [
        (int(rng.integers(40, 140)), int(rng.integers(1, 30))) for _ in range(2)], seed=5)
    want = check(index, from_spans(spans_of), len(spans_of), table, m=1, partial=True)
    one_word = want[2][(want[2]["line"] >= 1) & (want[2]["line"] <= 64)]
    assert len(one_word) > 300 and (one_word["covered"] == 1).all()
    assert (one_word["first"] == one_word["last"]).all() and (one_word["runs"] == 1).all()
    assert (want[0]["works"][1:65] == want[0]["whole_works"][1:65]).all()


# ---- active works: the edges of a column of 64 ----------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 129])
def test_active_works_around_a_column(index, n_active):
    cols, n_works = random_works(n_active, seed=n_active, lo=3, hi=60, most=4)
    assert n_works > n_active                              # active numbers are not work numbers
    table = random_table(seed=n_active)
    want = check(index, cols, n_works, table, m=3, runs2=n_active > 1)
    assert len(want[1]) == n_active
    assert (np.diff(want[1]["work"].astype(np.int64)) > 0).all()
    # the last active work, the last lane of the last column, quotes the first line whole
    last = int(cols[0].max())
    more = from_spans([[]] * last + [[(0, table[1] + 3)]])
    keep = cols[0] != last
    cols = tuple(np.concatenate([c[keep], x]) for c, x in zip(cols, more))
    want = check(index, cols, n_works, table, m=3, g=1, most=80)
    mine = want[2][want[2]["work"] == last]
    assert mine["line"].tolist()[0] == 0 and mine["covered"][0] == table[1]
    assert want[1]["work"][-1] == last and len(want[1]) == n_active


# ---- chunks of lines ------------------------------------------------------------------------

@pytest.mark.parametrize("n_lines", [1, 3, 4, 5, 9])
def test_lines_around_a_chunk_of_four(index, n_lines, monkeypatch):
    monkeypatch.setenv("FS_LINES_CHUNK", "4")
    width = N_SCRIPT // n_lines
    table = [l * width for l in range(n_lines)] + [N_SCRIPT]
    cols, n_works = random_works(70, seed=40 + n_lines, lo=3, hi=900, most=3)
    check(index, cols, n_works, table, m=3, whole=n_lines > 5, runs2=True)


def test_a_monologue_across_a_chunk_edge_a_work_on_every_line_and_a_line_nobody_touches(
        index, monkeypatch):
    monkeypatch.setenv("FS_LINES_CHUNK", "4")
    # lines of 10 words; line 3 (the last of chunk 0) is a monologue of 300; line 7 is skipped
    table = [0, 10, 20, 30, 330] + [340 + 10 * k for k in range(20)] + [N_SCRIPT]
    spans_of = interleaved(66, lambda k, rng: (
        [(0, 360), (370, N_SCRIPT - 370)] if k else [(0, N_SCRIPT)]), seed=2)
    spans_of[-1] = [(25, 100), (200, 135)]               # the monologue in two pieces
    first_active = next(w for w, s in enumerate(spans_of) if s and s[0][1] > 2)
    want = check(index, from_spans(spans_of), len(spans_of), table, m=3, runs2=True)
    found, works, cells = want
    assert found["works"][7] == 1 and found["first_work"][7] == first_active   # line 7: 360..369
    assert (found["works"][[6, 8]] == 66).all() and found["works"][3] == 67
    assert works["lines"][0] == len(table) - 1 == works["whole_lines"][0]
    assert (works["top_line"][:-1] == len(table) - 2).all()    # the rest of the script
    mono = cells[(cells["line"] == 3) & (cells["work"] == len(spans_of) - 1)]
    assert mono[["covered", "first", "last", "runs"]].tolist() == [(225, 30, 329, 2)]


def test_the_walk_without_the_skip_and_with_other_chunks_gives_the_same(index, monkeypatch):
    cols, n_works = random_works(129, seed=77, lo=3, hi=80, most=4)
    table = random_table(seed=77)
    want = check(index, cols, n_works, table, m=3, runs2=True)
    assert len(table) > 200
    for skip, chunk in (("0", None), ("0", "4"), ("1", "1"), ("1", "255"), ("1", "0")):
        monkeypatch.setenv("FS_LINES_SKIP", skip)
        if chunk is None:
            monkeypatch.delenv("FS_LINES_CHUNK", raising=False)
        else:
            monkeypatch.setenv("FS_LINES_CHUNK", chunk)
        assert_equal(check(index, cols, n_works, table, m=3), want)
    L = _lib.load()
    ms = (C.c_double * 3)()
    assert L.fs_lines_times(ms) == abi.FS_OK and ms[0] > 0 and ms[1] > 0
    assert abs(ms[2] - ms[0] - ms[1]) < 1e-9


# ---- --most ---------------------------------------------------------------------------------

def test_most_at_its_ends_and_exactly_at_the_bound(index):
    # lines of 3 words; work 0 covers 2 of line 0's 3 words, work 1 all of it
    table = list(range(0, N_SCRIPT + 1, 3))
    cols = from_spans([[(0, 2), (30, 5)], [(0, 3)], [(31, 1)]])
    counted = {}
    for most in (1, 66, 67, 100):
        want = check(index, cols, 3, table, m=1, most=most)
        counted[most] = int(want[0]["most_works"][0])
        assert want[0]["works"][0] == 2 and want[0]["whole_works"][0] == 1
    # 2 * 100 = 200 >= 66 * 3 = 198, and 200 < 67 * 3 = 201
    assert counted == {1: 2, 66: 2, 67: 1, 100: 1}
    want = check(index, cols, 3, table, m=1, most=1)
    assert (want[0]["most_works"] == want[0]["works"]).all()
    want = check(index, cols, 3, table, m=1, most=100)
    assert (want[0]["most_works"] == want[0]["whole_works"]).all()


# ---- capacities, errors and edges -----------------------------------------------------------

def _call(L, cols, n_works, table, m, most, found, works, w_cap, n_active, cells, c_cap, n_cells,
          n_rows=None, n_script=N_SCRIPT):
    table = np.ascontiguousarray(table, dtype=np.uint32)
    return L.fs_lines(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                      abi.ptr(cols[2], C.c_uint32), len(cols[0]) if n_rows is None else n_rows,
                      n_works, n_script, abi.ptr(table, C.c_uint32), len(table) - 1, m, 0, most,
                      found.ctypes.data_as(C.c_void_p),
                      works.ctypes.data_as(C.c_void_p) if w_cap else None, w_cap,
                      C.byref(n_active),
                      cells.ctypes.data_as(C.c_void_p) if c_cap else None, c_cap,
                      C.byref(n_cells))


def test_capacities_too_small_exact_and_grown(index, monkeypatch):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols, n_works = random_works(100, seed=8, hi=60)
    cols = [np.ascontiguousarray(c) for c in cols]
    table = random_table(seed=8)
    n_lines = len(table) - 1
    want = oracle(cols, n_works, table, 3, 0, 50)
    na, nc = len(want[1]), len(want[2])
    assert na == 100 and nc > 300
    L = _lib.load()
    found = np.zeros(n_lines, dtype=abi.LINE_DTYPE)
    works = np.zeros(na, dtype=abi.LINE_WORK_DTYPE)
    cells = np.zeros(nc, dtype=abi.LINE_CELL_DTYPE)
    n_active, n_cells = C.c_uint64(0), C.c_uint64(0)
    for w_cap, c_cap in ((na, 0), (na, nc - 1), (na - 1, nc), (0, 0)):
        found[:] = 0
        rc = _call(L, cols, n_works, table, 3, 50, found, works, w_cap, n_active, cells, c_cap,
                   n_cells)
        assert rc == abi.FS_E_CAPACITY and (n_active.value, n_cells.value) == (na, nc)
        assert_equal((found,), want[:1])                   # the lines are complete
        assert not works["lines"].any() and not cells["covered"].any()     # the rest untouched
    assert _call(L, cols, n_works, table, 3, 50, found, works, na, n_active, cells, nc,
                 n_cells) == abi.FS_OK
    assert (n_active.value, n_cells.value) == (na, nc)
    assert_equal((found, works, cells), want)
    # find_lines begins with room for 256 works and 4096 cells and grows; a roomy first call
    assert nc < 4096
    assert_equal(lines.find_lines(*cols, n_works, N_SCRIPT, table, 3), want)
    more, n_more = random_works(300, seed=9, hi=200, most=5)
    big = oracle(more, n_more, table, 3, 0, 50)
    assert len(big[1]) == 300 and len(big[2]) > 4096       # both buffers grow
    assert_equal(lines.find_lines(*more, n_more, N_SCRIPT, table, 3), big)
    # the caller's own device buffers
    d_rows, d_table = on_device(cols, table)
    d_lines = torch.zeros(n_lines * 32, dtype=torch.uint8, device="cuda")
    d_works = torch.zeros(na * 32, dtype=torch.uint8, device="cuda")
    d_cells = torch.zeros(nc * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_lines.data_ptr(), d_works.data_ptr(), d_cells.data_ptr())
    args = (d_rows.data_ptr(), len(cols[0]), n_works, d_table.data_ptr(), n_lines, 3, 0, 50)
    for caps in ((na, nc - 1), (na - 1, nc), (na, 0)):
        with pytest.raises(_lib.FsError) as e:
            index.lines_device(*args, out_ptrs=ptrs, caps=caps)
        assert e.value.code == abi.FS_E_CAPACITY and e.value.required == (na, nc)
        assert (d_lines.cpu().numpy().view(abi.LINE_DTYPE) == want[0]).all()
        assert not d_works.cpu().numpy().any() and not d_cells.cpu().numpy().any()
    assert index.lines_device(*args, out_ptrs=ptrs, caps=(na, nc)) == (na, nc)
    assert (d_works.cpu().numpy().view(abi.LINE_WORK_DTYPE) == want[1]).all()
    assert (d_cells.cpu().numpy().view(abi.LINE_CELL_DTYPE) == want[2]).all()
    # no records on the device: lines nobody quotes
    assert index.lines_device(d_rows.data_ptr(), 0, n_works, d_table.data_ptr(), n_lines, 3, 0, 50,
                              out_ptrs=ptrs, caps=(na, nc)) == (0, 0)
    none = d_lines.cpu().numpy().view(abi.LINE_DTYPE)
    assert (none["first_work"] == NONE).all() and not none["works"].any()
    assert not none["covered_sum"].any()


def test_no_records_one_line_and_no_passage(index):
    empty = (np.zeros(0, np.uint32),) * 3
    table = random_table(seed=1)
    found, works, cells = check(index, empty, 3, table, whole=False, partial=False)
    assert len(works) == 0 and len(cells) == 0
    assert found.tolist() == [(0, 0, 0, 0, 0, NONE, 0)] * (len(table) - 1)
    cols, n_works = random_works(10, seed=2)
    found, works, cells = check(index, cols, n_works, [0, N_SCRIPT], whole=False)   # one line
    assert len(found) == 1 and found["works"][0] == 10 == len(cells)
    assert (works["top_line"] == 0).all() and (works["line_words"] == N_SCRIPT).all()
    whole = from_spans([[(0, N_SCRIPT)]])
    found, _, cells = check(index, whole, 1, [0, N_SCRIPT], partial=False)
    assert cells.tolist() == [(0, 0, N_SCRIPT, 0, N_SCRIPT - 1, 1, 0, 0)]
    found, works, cells = check(index, cols, n_works, table, m=41, whole=False, partial=False)
    assert len(works) == 0 and len(cells) == 0 and not found["works"].any()


def test_refusals(index):
    from fandom_search_amd.engine import torch_ready
    from tests.test_gpu_pairs import records
    cols = records([300, 500, 200], N_SCRIPT, seed=9)
    table = random_table(seed=9)

    def refused(c, n_works=3, table=table, m=6, most=50, code=abi.FS_E_INVALID,
                n_script=N_SCRIPT, rows=True):
        with pytest.raises(_lib.FsError) as e:
            lines.find_lines(*c, n_works, n_script, table, m, 0, most)
        assert e.value.code == code
        if rows:
            d_rows, d_table = on_device(c, table)
            torch_ready()
            with pytest.raises(_lib.FsError) as e:
                index.lines_device(d_rows.data_ptr(), len(c[0]), n_works, d_table.data_ptr(),
                                   len(table) - 1, m, 0, most)
            assert e.value.code == code
    refused(cols, m=0)
    refused(cols, most=0)
    refused(cols, most=101)
    refused(cols, n_works=2)                               # a work >= n_works
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    for bad in ([1] + table[1:],                           # does not start at 0
                table[:-1] + [N_SCRIPT - 1],               # does not end at n_script
                table[:-1] + [N_SCRIPT + 1],
                table[:5] + [table[4]] + table[5:],        # an empty line
                table[:5] + [table[6], table[5]] + table[7:]):     # descending
        refused(cols, table=bad)
    big = [0, (1 << 19) + 1]
    refused(cols, table=big, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED, rows=False)
    L = _lib.load()
    n_active, n_cells = C.c_uint64(0), C.c_uint64(0)
    found = np.zeros(len(table) - 1, dtype=abi.LINE_DTYPE)
    rc = _call(L, cols, 3, table, 6, 50, found, found, 0, n_active, found, 0, n_cells,
               n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(index, cols, 3, table, m=6)                      # and the same columns are accepted


# ---- the counts of the sibling commands on the same records -------------------------------

def test_works_of_a_line_are_those_of_companions_and_covered_is_that_of_pairs(index):
    cols, n_works = random_works(70, seed=31, hi=90, most=4)
    table = random_table(seed=31)
    n_lines = len(table) - 1
    found, works, cells = lines.find_lines(*cols, n_works, N_SCRIPT, table, 3, 1, 50)
    line_of = np.repeat(np.arange(n_lines, dtype=np.uint32), np.diff(table))
    units, _ = companions.find_companions(*cols, n_works, N_SCRIPT, line_of, n_lines, 3, 1,
                                          min_both=1 << 30)
    assert (found["works"] == units["works"]).all() and found["works"].sum() > 500
    pair_works, _ = pairs.find_pairs(*cols, n_works, N_SCRIPT, 3, 1, 1 << 30)
    assert len(works) == 70
    assert (pair_works["covered"][works["work"]] == works["covered"]).all()
    assert pair_works["covered"].sum() == works["covered"].sum() == cells["covered"].sum()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,m,g,k,most", mlg.CASES)
def test_command_on_the_golden_input(tmp_path, case, m, g, k, most, reader):
    src, markup = os.path.join(GOLDEN, mlg.INPUT), os.path.join(GOLDEN, mlg.MARKUP)
    prefix = str(tmp_path / "p")
    assert main(["lines", src, markup, "-o", prefix, "--min-words", str(m), "--max-gap", str(g),
                 "--min-works", str(k), "--most", str(most), "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in lines.output_names(src, prefix))
    with open(src, newline="", encoding="utf-8") as fh:
        want = lr.lines_csv(fh.read(), mlg.SCRIPT, m, g, k, most)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mlg.golden_names(case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


@pytest.mark.parametrize("reader", ["device", "python"])
def test_command_refuses_another_script_s_records_and_takes_the_default_prefix(tmp_path, reader):
    import shutil
    src, markup = str(tmp_path / "m.csv"), str(tmp_path / "s.txt")
    shutil.copy(os.path.join(GOLDEN, mlg.INPUT), src)
    with open(markup, "w", encoding="utf-8") as fh:
        fh.write(mlg.SCRIPT)
    assert main(["lines", src, markup, "--reader", reader]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        text = fh.read()
    for path, part in zip(lines.output_names(src), lr.lines_csv(text, mlg.SCRIPT)):
        with open(path, "rb") as fh:
            assert fh.read() == part.encode("utf-8"), path
    other = mlg.SCRIPT.replace("a bad feeling", "a good feeling")
    with open(markup, "w", encoding="utf-8") as fh:
        fh.write(other)
    with pytest.raises(SystemExit) as e:
        main(["lines", src, markup, "--reader", reader])
    assert str(e.value.code) == (
        "ao3.py lines: error: script word 7 is 'bad' in the records and 'good' in the script "
        "markup: was the file searched against another script?")
    with open(markup, "w", encoding="utf-8") as fh:
        fh.write(mlg.SCRIPT[:mlg.SCRIPT.index("CHARACTER_NAME<<LUKE>>\nLINE<<may")])
    with pytest.raises(SystemExit) as e:
        main(["lines", src, markup, "--reader", reader])
    assert str(e.value.code).startswith(
        "ao3.py lines: error: ORIGINAL_SCRIPT_WORD_INDEX 67 in a script markup of 62 words (the "
        "records need at least 68)")
