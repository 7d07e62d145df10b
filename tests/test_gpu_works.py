"""`works` on the GPU: fs_works / fs_works_rows against the restated contract
(tests/works_restated.py), every figure compared for equality; works of every size the
kernels treat differently; the planted copies of a synthetic corpus after a real search;
`ao3.py works` byte for byte against the oracle's three files."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, synth, works
from fandom_search_amd.cli import main
from tests import works_restated as wr
from tests.golden import make_works_golden as mwg
from tests.test_gpu_passages import expected_spans, repeated_ngrams

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# records of a work one wave reduces; longer works are cut into slices.  Doubled until it is at
# least the words of a work's merge area, n_script / 32 + 2 * n_groups (16384 and 32768 at the
# limits below)
SLICE = 8192
WORKS_PER_WAVE = 8          # consecutive works a wave takes from MANY_WORKS works on, one below
MANY_WORKS = 1 << 18
THR = wr.THRESHOLDS


def oracle(cols, n_works, n_script, group_of, n_groups, m, g, thr=THR):
    work, fan, orig, comb = cols
    recs = list(zip(work.tolist(), fan.tolist(), orig.tolist(), [0.0] * len(work), comb.tolist()))
    out, counts, cells = wr.works(recs, n_works, n_script,
                                  None if group_of is None else list(map(int, group_of)),
                                  n_groups, m, g, thr)
    o = np.zeros(n_works, dtype=abi.WORK_DTYPE)
    for k, d in enumerate(out):
        for name in wr.WORK_KEYS:
            o[name][k] = d[name]
    c = np.array(counts, dtype=np.uint32).reshape(n_works, len(thr) + 1)
    x = np.array(cells, dtype=np.uint32).reshape(-1, 4)
    return o, c, np.ascontiguousarray(x).view(abi.WORK_CELL_DTYPE).reshape(-1)


def assert_equal(got, want):
    for a, b, dt in zip(got[::2], want[::2], (abi.WORK_DTYPE, abi.WORK_CELL_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])
    assert got[1].shape == want[1].shape
    bad = np.argwhere(got[1] != want[1])
    assert bad.size == 0, (bad[0], got[1][bad[0][0]], want[1][bad[0][0]])


def records(sizes, n_script, seed, cont=0.8, nan=0.02):
    """Records sorted by (work, fan_ix), sizes[w] of them in work w: diagonal steps most of the
    time, repeats, jumps, NaN, -0.0 and 0.0, script indices below n_script."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n = int(sizes.sum())
    work = np.repeat(np.arange(len(sizes)), sizes)
    fstep = rng.choice([0, 1, 2, 3], size=n, p=[0.05, 0.8, 0.1, 0.05])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < cont, fstep, rng.integers(-50, 50, size=n))
    orig = (np.cumsum(ostep) + int(rng.integers(0, 1 << 20))) % n_script
    comb = np.round(rng.random(n) * 0.6, 2) * rng.integers(0, 2, size=n)
    r = rng.random(n)
    comb[r < nan] = np.nan
    comb[(r >= nan) & (r < 2 * nan)] = -0.0
    comb[(r >= 2 * nan) & (r < 3 * nan)] = 0.05
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), comb


def group_map(n_script, n_groups, seed):
    """Scenes: stretches of the script, in no order of id."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, n_script, size=max(0, n_groups - 1)))
    ids = rng.permutation(n_groups)
    return ids[np.searchsorted(cuts, np.arange(n_script), side="right")].astype(np.uint32)


def check(cols, n_works, n_script, group_of, n_groups, m=6, g=0, thr=THR):
    got = works.summarise(*cols, n_works, n_script, group_of, n_groups, m, g, thr)
    assert_equal(got, oracle(cols, n_works, n_script, group_of, n_groups, m, g, thr))
    return got


def test_no_records_and_one_record():
    empty = (np.zeros(0, np.uint32),) * 3 + (np.zeros(0),)
    out, counts, cells = check(empty, 3, 10, np.zeros(10, np.uint32), 2)
    assert len(out) == 3 and (out["top_group"] == abi.FS_NONE).all() and len(cells) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32),
           np.array([-0.0]))
    out, counts, cells = check(one, 3, 10, np.arange(10, dtype=np.uint32) % 4, 4, m=1)
    assert counts[1].tolist() == [1] * 12 and cells.tolist() == [(1, 1, 1, 1)]
    assert out["n_passages"].tolist() == [0, 1, 0]


def test_random_records_over_the_parameters():
    rng = np.random.default_rng(2025)
    for k in range(10):
        n_works = int(rng.integers(1, 400))
        sizes = rng.integers(0, 300, size=n_works) * (rng.random(n_works) < 0.8)
        n_script = int(rng.integers(1, 30_000))
        n_groups = int(rng.integers(1, 400))
        cols = records(sizes, n_script, seed=k, cont=float(rng.random()),
                       nan=float(rng.random()) * 0.2)
        m, g = int(rng.integers(1, 13)), int(rng.integers(0, 4))
        check(cols, n_works, n_script, group_map(n_script, n_groups, k), n_groups, m, g)
        check(cols, n_works, n_script, None, 0, m, g)
    # other thresholds: one, and sixty-four
    cols = records([500, 0, 700], 2000, seed=77)
    check(cols, 3, 2000, group_map(2000, 30, 1), 30, 3, 1, thr=[0.25])
    check(cols, 3, 2000, group_map(2000, 30, 1), 30, 3, 1, thr=[k / 100 for k in range(64)])


def test_a_hundred_thousand_small_works():
    rng = np.random.default_rng(5)
    sizes = rng.integers(1, 6, size=100_000)
    cols = records(sizes, 20_000, seed=5)
    out, _, cells = check(cols, len(sizes), 20_000, group_map(20_000, 300, 5), 300, m=3)
    assert (out["n_words"] == sizes).all() and len(cells) >= len(sizes)


def test_one_work_of_three_million_records():
    n = 3_000_000
    cols = records([0, n, 0], 20_000, seed=3, cont=0.97)
    gmap = group_map(20_000, 300, 3)
    out, _, cells = check(cols, 3, 20_000, gmap, 300)
    assert out["n_words"].tolist() == [0, n, 0] and out["n_script_words"][1] == 20_000
    assert out["longest"][1] >= 6 and len(cells) == len(np.unique(gmap))   # every word is hit


@pytest.mark.parametrize("size", [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE,
                                  2 * SLICE + 1, 5 * SLICE + 3])
def test_works_that_end_around_a_slice(size):
    # the work alone; between small works, so that it starts anywhere in a slice; and twice in
    # a row, so that one slice holds the end of one large work and the start of the next
    for sizes in ([size], [3, 0, size, 5], [SLICE // 2 + 1, size, size, 2, SLICE + 1, 7]):
        cols = records(sizes, 5000, seed=size, cont=0.9)
        check(cols, len(sizes), 5000, group_map(5000, 100, size), 100)


@pytest.mark.parametrize("n_works", [1, WORKS_PER_WAVE - 1, WORKS_PER_WAVE, WORKS_PER_WAVE + 1,
                                     64, 65, 1024, 1025, 3000, 4095, 4096, 4097,
                                     MANY_WORKS - 1, MANY_WORKS, MANY_WORKS + WORKS_PER_WAVE + 1])
def test_numbers_of_works_around_a_wave_share(n_works):
    rng = np.random.default_rng(n_works)
    sizes = rng.integers(0, 40 if n_works < 10_000 else 4, size=n_works)
    cols = records(sizes, 3000, seed=n_works)
    check(cols, n_works, 3000, group_map(3000, 70, n_works), 70, m=2, g=1)


@pytest.mark.parametrize("n_script", [1, (1 << 19) - 1, 1 << 19])
def test_script_sizes_up_to_the_limit(n_script):
    cols = records([40, 20_000, 0, 3, 16_384, 16_385], n_script, seed=n_script)
    check(cols, 6, n_script, group_map(n_script, 50, 2), 50)
    if n_script > 1:                                    # the last script word, too
        cols[2][-1] = n_script - 1
        cols[2][5] = n_script - 1
        out, _, _ = check(cols, 6, n_script, None, 0, m=1)
        distinct = len(np.unique(cols[2][40:20_040]))
        assert out["n_script_words"][1] == distinct and distinct > 5_000


@pytest.mark.parametrize("n_groups", [1, 4096])
def test_group_counts_up_to_the_limit(n_groups):
    cols = records([40, 70_000, 0, 3], 1 << 19, seed=n_groups, cont=0.2)
    group_of = (np.arange(1 << 19, dtype=np.uint32) * 7) % n_groups
    out, _, cells = check(cols, 4, 1 << 19, group_of, n_groups)
    assert out["n_groups_hit"][1] == (1 if n_groups == 1 else len(set(group_of[cols[2][40:70_040]])))


def test_past_the_limits_is_refused():
    """include/fandom_search.h: n_script > FS_WORKS_MAX_SCRIPT or n_groups > FS_WORKS_MAX_GROUPS
    is FS_E_UNSUPPORTED (no slower form)."""
    cols = records([100], 1000, seed=1)
    for n_script, n_groups in (((1 << 19) + 1, 10), (1000, 4097)):
        with pytest.raises(_lib.FsError) as e:
            works.summarise(*cols, 1, n_script, np.zeros(n_script, np.uint32), n_groups)
        assert e.value.code == abi.FS_E_UNSUPPORTED


def test_refusals():
    cols = records([3000, 5000, 2000], 1000, seed=9)
    gmap = group_map(1000, 10, 9)

    def refused(c, n_works=3, n_script=1000, group_of=gmap, n_groups=10, m=6):
        with pytest.raises(_lib.FsError) as e:
            works.summarise(*c, n_works, n_script, group_of, n_groups, m)
        assert e.value.code == abi.FS_E_INVALID
    refused(cols, m=0)
    refused(cols, n_works=2)                               # a work >= n_works
    refused(cols, n_script=int(cols[2].max()), group_of=gmap[:int(cols[2].max())])
    bad = gmap.copy()
    bad[500] = 10
    refused(cols, group_of=bad)
    fan = cols[1].copy()
    fan[7000], fan[7001] = fan[7001] + 1, fan[7000]
    refused((cols[0], fan, cols[2], cols[3]))
    work = cols[0].copy()
    work[9000] = 0
    refused((work, np.arange(10_000, dtype=np.uint32), cols[2], cols[3]))
    check(cols, 3, 1000, gmap, 10)                         # and the same columns are accepted


def test_capacity_too_small_by_one_exact_and_zero():
    cols = [np.ascontiguousarray(c) for c in records([300, 0, 4000, 20_000], 3000, seed=8)]
    gmap = group_map(3000, 40, 8)
    want = oracle(cols, 4, 3000, gmap, 40, 6, 0)
    k = len(want[2])
    assert k > 40
    L = _lib.load()
    thr = np.array(THR)
    out = np.zeros(4, dtype=abi.WORK_DTYPE)
    counts = np.zeros((4, 12), dtype=np.uint32)
    cells = np.zeros(k, dtype=abi.WORK_CELL_DTYPE)
    n = C.c_uint64(0)

    def call(cap):
        return L.fs_works(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                          abi.ptr(cols[2], C.c_uint32), abi.ptr(cols[3], C.c_double), len(cols[0]),
                          4, 3000, abi.ptr(gmap, C.c_uint32), 40, 6, 0, abi.ptr(thr, C.c_double),
                          len(thr), out.ctypes.data_as(C.c_void_p),
                          counts.ctypes.data_as(C.c_void_p),
                          cells.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))
    for cap in (k - 1, 0):
        out[:] = 0
        counts[:] = 0
        assert call(cap) == abi.FS_E_CAPACITY and n.value == k
        assert_equal((out, counts, want[2]), want)         # summaries and counts are complete
        assert not cells["n_words"].any()
    assert call(k) == abi.FS_OK and n.value == k
    assert_equal((out, counts, cells), want)


# ---- after a real search ---------------------------------------------------------------

def test_device_rows_after_a_search(synth_base):
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    words, emb = synth_base["words"], synth_base["emb"]
    n_works, per, n = 300, 2000, 6
    script = synth.script_tokens(5000)
    tok, off = synth.corpus_tokens(n_works, per, script)
    ix = ScriptIndex(script, [words[int(t)] for t in script], emb, synth.lsh_normals(n))
    corpus = ix.corpus(tok, off, synth_base["chars"], synth_base["off"])
    cap = len(tok) // 4
    buf = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    n_rows, _ = ix.search_device(corpus, buf.data_ptr(), cap)
    rows = buf[:n_rows * 32].cpu().numpy().view(abi.ROW_DTYPE)
    cols = tuple(np.ascontiguousarray(rows[c]) for c in ("work", "fan_ix", "orig_ix", "comb"))
    gmap = group_map(len(script), 60, 4)
    for group_of, n_groups, g in ((gmap, 60, 0), (gmap, 60, 1), (None, 0, 0)):
        dev = ix.works_device(buf.data_ptr(), n_rows, n_works, group_of, n_groups, n, g)
        host = works.summarise(*cols, n_works, len(script), group_of, n_groups, n, g)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, len(script), group_of, n_groups, n, g))
    # the caller's own device buffers, the cells' too small first
    k = len(host_cells := works.summarise(*cols, n_works, len(script), gmap, 60, n, 0)[2])
    d_out = torch.zeros(n_works * 56, dtype=torch.uint8, device="cuda")
    d_counts = torch.zeros(n_works * 12, dtype=torch.int32, device="cuda")
    d_cells = torch.zeros(k * 16, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_out.data_ptr(), d_counts.data_ptr(), d_cells.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        ix.works_device(buf.data_ptr(), n_rows, n_works, gmap, 60, n, 0, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert ix.works_device(buf.data_ptr(), n_rows, n_works, gmap, 60, n, 0, out_ptrs=ptrs,
                           cap=k) == k
    assert (d_cells.cpu().numpy().view(abi.WORK_CELL_DTYPE) == host_cells).all()
    # every planted copy is inside its work's figures
    out = dev[0]
    checked = 0
    repeated = repeated_ngrams(script, n)
    for w in range(n_works):
        for dst, length, src in expected_spans(w, per, script, n, repeated)[0]:
            assert out["n_script_words"][w] >= length and out["longest"][w] >= length, (w, dst)
            checked += 1
    assert checked > 200
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

def _run_command(tmp_path, src_path, m, g):
    prefix = str(tmp_path / "w")
    assert main(["works", src_path, "-o", prefix, "--min-words", str(m), "--max-gap", str(g)]) == 0
    return tuple(open(p, "rb").read() for p in works.output_names(src_path, prefix))


@pytest.mark.parametrize("case,src,m,g", mwg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g):
    got = _run_command(tmp_path, os.path.join(GOLDEN, src), m, g)
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        want = wr.works_csv(fh.read(), m, g)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mwg.golden_names(case, m, g), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_search_then_works(tmp_path, monkeypatch, synth_base):
    from fandom_search_amd import search
    words = synth_base["words"]
    n_works, per = 40, 1500
    script = synth.script_tokens(3000)
    fandir = tmp_path / "fanworks"
    synth.write_corpus(str(fandir), n_works, per, script, words)
    (tmp_path / "script.txt").write_text(synth.script_markup(script, words))
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    monkeypatch.delenv("FANDOM_SEARCH_VECTORS", raising=False)
    assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--synthetic-vocab"]) == 0
    dated = "match-6gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    assert main(["works", dated]) == 0                     # default prefix: beside the input
    with open(dated, newline="", encoding="utf-8") as fh:
        want = wr.works_csv(fh.read())
    for path, text in zip(works.output_names(dated), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[0].count("\r\n") > 10 and want[1].count("\r\n") > 10
