"""`ao3.py alignments` on the GPU: fs_alignments and fs_alignments_rows against the plain-Python
restatement (tests/alignments_restated.py), every field of every fs_alignment and the whole
path list compared for equality, every case with the segments sent down each path in turn
(FS_ALIGNMENTS_SMALL, FS_ALIGNMENTS_RING) and through both entry points; and the command under
both readers against the committed expected CSVs."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, alignments, passages, synth
from fandom_search_amd.cli import main
from tests import alignments_restated as ar
from tests.golden import make_alignments_golden as mag

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HUGE = str(1 << 31)
# (FS_ALIGNMENTS_SMALL, FS_ALIGNMENTS_RING): the defaults; every segment by a wave; every
# segment by a single lane; every segment by a wave that keeps no ring
PATHS = {"default": (None, None), "wave": ("0", None), "lane": (HUGE, None), "noring": ("0", "0")}
LENGTHS = [1, 2, 8, 9, 63, 64, 65, 66, 128, 129, 300, 5000]
SHAPES = ["diagonal", "indels", "strays", "random"]
REACHES = [0, 1, 4, 62, 63]


@pytest.fixture(params=list(PATHS), ids=list(PATHS))
def path(request, monkeypatch):
    for name, value in zip(("FS_ALIGNMENTS_SMALL", "FS_ALIGNMENTS_RING"), PATHS[request.param]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


@pytest.fixture(scope="module")
def index(synth_base):
    """An index for fs_alignments_rows to take its device and stream from."""
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(3000)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def columns(records):
    """(work, fan_ix, orig_ix, comb) arrays of (work, fan, orig, comb) tuples."""
    work, fan, orig, comb = zip(*records) if records else ((), (), (), ())
    return (np.asarray(work, dtype=np.uint32), np.asarray(fan, dtype=np.uint32),
            np.asarray(orig, dtype=np.uint32), np.asarray(comb, dtype=np.float64))


def oracle(cols, m=6, r=4, s=2, p=1):
    found, walk = ar.alignments(list(zip(*(c.tolist() for c in cols))), m, r, s, p)
    a = np.array([tuple(x[k] for k in ar.KEYS) for x in found], dtype=abi.ALIGNMENT_DTYPE)
    return a, np.asarray(walk, dtype=np.uint32)


def assert_equal(got, want):
    (a, walk), (b, want_walk) = got, want
    assert a.dtype == abi.ALIGNMENT_DTYPE and len(a) == len(b), (len(a), len(b))
    for name in abi.ALIGNMENT_DTYPE.names:                     # (the reserved word, 0, too)
        bad = np.flatnonzero(a[name] != b[name])
        assert not len(bad), (name, bad[:5], a[name][bad[:5]], b[name][bad[:5]])
    assert walk.dtype == np.uint32 and len(walk) == len(want_walk)
    bad = np.flatnonzero(walk != want_walk)
    assert not len(bad), (bad[:5], walk[bad[:5]], want_walk[bad[:5]])


def on_device(cols):
    import torch
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix", "comb"), cols):
        rows[name][:len(col)] = col
    return torch.from_numpy(rows.view(np.uint8)).to("cuda")


def check(index, cols, m=6, r=4, s=2, p=1, want=None):
    """Both entry points against the restatement; the host entry point's result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, m, r, s, p) if want is None else want
    got = alignments.find_alignments(*cols, m, r, s, p)
    assert_equal(got, want)
    d_rows = on_device(cols)
    torch_ready()
    assert_equal(index.alignments_device(d_rows.data_ptr(), len(cols[0]), m, r, s, p), want)
    return got


# ---- one segment of L records ----------------------------------------------------------------

def shape(kind, n):
    """n records of one work; comb 0, 0.25 and NaN in turn."""
    rng = np.random.default_rng(n)
    out, fan, orig = [], 7, 1000
    for k in range(n):
        comb = (0.0, 0.25, float("nan"))[k % 3]
        if kind == "strays" and k % 4 == 3:
            out.append((0, fan, 50 + (k * 37) % 400, comb))   # points elsewhere
        elif kind == "random":
            out.append((0, fan, orig + (int(rng.integers(-2, 3)) if rng.random() < 0.2 else 0), comb))
        else:
            out.append((0, fan, orig, comb))
        fan += 1
        orig += 1
        if kind == "indels" and k % 5 == 4:
            if k % 10 == 4:
                fan += 1                                      # an inserted word
            else:
                orig += 1                                     # a dropped word
        if kind == "random" and rng.random() < 0.25:
            fan += int(rng.integers(-1, 2))                   # the same fan index again, or a gap
            orig += int(rng.integers(-1, 3))
    return out


@functools.lru_cache(maxsize=None)
def one_segment(kind, n):
    cols = columns(shape(kind, n))
    return cols, {r: oracle(cols, 3, r) for r in REACHES}


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("kind", SHAPES)
def test_one_segment_of_n_records(index, path, kind, n):
    cols, wants = one_segment(kind, n)
    for r in REACHES:
        found, walk = check(index, cols, 3, r, want=wants[r])
        if kind == "diagonal":
            assert len(found) == (n >= 3) and found["n_words"].sum() == (n if n >= 3 else 0)
        if kind == "indels" and r >= 1 and n >= 3:
            assert len(found) == 1 and found["n_words"][0] == n
            assert found["fan_skipped"][0] + found["orig_skipped"][0] == (n - 1) // 5
        if kind == "strays" and r >= 1 and n >= 5:
            # the strays are stepped over; a last record right behind one only ties the peak
            assert found["n_words"].max() == n - n // 4 - (n % 4 == 1)
        if r == 0 and kind != "random":                       # (no two records at one fan index)
            same = passages.find_passages(cols[0], cols[1], cols[2], cols[3], cols[3], 3, 0)
            for name in ("first", "n_words", "n_exact"):
                assert found[name].tolist() == same[name].tolist(), name
            assert (found["pieces"] == 1).all() and (found["tree_records"] == found["n_words"]).all()


# ---- a predecessor at the far edge of reach --------------------------------------------------

@pytest.mark.parametrize("side", ["fan", "script"])
def test_the_best_predecessor_at_the_far_edge_of_reach(index, path, side):
    """R = 63, links free.  A is the last of a run of ten records, B a root beside it.  The
    target lies R + 1 past B and R + 2 past A on `side`, and records that link to nothing lie
    between: the target takes B, the worse one, and A is ignored."""
    if side == "fan":
        run = [(0, 10 + k, 200 + k, 0.0) for k in range(10)]      # A: fan 19
        b = [(0, 20, 150, 0.0)]                                    # B: fan 20, in front of the run in the script
        fill = [(0, 21 + k, 9000 - k, 0.0) for k in range(63)]
        recs, at_b = run + b + fill + [(0, 84, 212, 0.0)], 10      # 64 fan words past B, 65 past A
    else:
        b = [(0, 9, 146, 0.0)]                                     # B: script 146, in front of the run
        run = [(0, 10 + k, 136 + k, 0.0) for k in range(10)]      # A: script 145
        fill = [(0, 21 + k, 9000 - k, 0.0) for k in range(20)]
        recs, at_b = b + run + fill + [(0, 41, 210, 0.0)], 0       # 64 script words past B, 65 past A
    cols = columns(recs)
    found, walk = check(index, cols, 1, 63, 2, 0)
    last = found[found["last"] == len(recs) - 1]
    assert len(last) == 1 and last["first"][0] == at_b
    assert (last["n_words"][0], last["score"][0]) == (2, 4)
    assert found["score"].max() == 20                              # the run, without the target


# ---- more records in reach than the ring holds -----------------------------------------------

@pytest.mark.parametrize("k", [65, 130])
def test_ring_overflow(index, path, k):
    """k records at one fan index, the next fan index holds one record; only the first of the k
    lies before it in the script."""
    recs = [(0, 5, 10, 0.0)] + [(0, 5, 500 + j, 0.0) for j in range(k - 1)] + [(0, 6, 11, 0.0)]
    found, walk = check(index, columns(recs), 2, 4)
    assert found.tolist() == [(0, k, 2, 2, 4, 0, 0, 1, 2, 0, 0)] and walk.tolist() == [0, k]
    # and a better one nearer, inside the ring, for the same record
    recs[k - 3] = (0, 5, 9, 0.0)
    recs[k - 2] = (0, 5, 10, 0.0)
    found, walk = check(index, columns(recs), 2, 4)
    assert walk.tolist() == [k - 2, k]


# ---- segment boundaries ----------------------------------------------------------------------

def test_segment_boundaries(index, path):
    a = [(0, 1 + k, 100 + k, 0.0) for k in range(3)]
    other = [(1, 4 + k, 103 + k, 0.0) for k in range(3)]       # another work: the indices go on
    found, _ = check(index, columns(a + other), 1)
    assert found["n_words"].tolist() == [3, 3]
    for r in (0, 1, 4, 63):
        near = [(0, 3 + r + 1 + k, 103 + k, 0.0) for k in range(3)]   # a fan gap of R + 1
        found, _ = check(index, columns(a + near), 1, r, 16, 0)
        assert found["n_words"].tolist() == [6] and found["fan_skipped"].tolist() == [r]
        far = [(0, 3 + r + 2 + k, 103 + k, 0.0) for k in range(3)]    # of R + 2: two segments
        found, _ = check(index, columns(a + far), 1, r, 16, 0)
        assert found["n_words"].tolist() == [3, 3]


# ---- many small segments beside one long one -------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(5)
    recs = []
    for w in range(3001):
        n = 3000 if w == 1500 else int(rng.integers(1, 13))
        fan, orig = int(rng.integers(0, 9)), int(rng.integers(0, 2000))
        for _ in range(n):
            recs.append((w, fan, orig, float(rng.choice([0.0, 0.5]))))
            kind = rng.random()
            fan += 1 if kind < 0.85 else int(rng.integers(0, 5 if n == 3000 else 8))   # (one segment)
            orig = orig + 1 if kind < 0.9 else max(0, orig + int(rng.integers(-3, 6)))
    cols = columns(recs)
    return cols, {m: oracle(cols, m) for m in (1, 6)}


@pytest.mark.parametrize("min_words", [1, 6])
def test_many_small_segments_beside_a_long_one(index, path, min_words):
    cols, wants = mixed()
    found, walk = check(index, cols, min_words, want=wants[min_words])
    assert len(found) > (3000 if min_words == 1 else 300)
    assert (cols[0][found["first"].astype(np.int64)] == 1500).any()
    if min_words == 1:                                         # every record is in one tree
        assert found["tree_records"].sum() == len(cols[0])


# fs_alignments.hip counts heads and kept roots per 256 records, and the one-workgroup scan takes
# 1024 such counts per chunk
def test_more_workgroups_than_a_chunk_of_the_scan(index, monkeypatch):
    for name in ("FS_ALIGNMENTS_SMALL", "FS_ALIGNMENTS_RING"):
        monkeypatch.delenv(name, raising=False)
    n = 1024 * 256 + 300
    i = np.arange(n, dtype=np.int64)
    orig = np.where(i % 5 == 3, 7, i % 5 + 20)                 # five to a work, one stray
    cols = tuple(np.asarray(c, dtype=np.uint32) for c in (i // 5, i % 5, orig)) + (np.zeros(n),)
    found, walk = check(index, cols, 3)
    # three words, then the stray; the fifth record costs what it scores and stays a side record
    assert len(found) == n // 5 + 1 and (found["n_words"] == 3).all()
    assert (found["tree_records"][:-1] == 4).all() and found["tree_records"][-1] == 3
    assert walk.tolist() == (found["first"][:, None] + np.arange(3)).ravel().tolist()


# ---- match and gap at their bounds -----------------------------------------------------------

@pytest.mark.parametrize("kind", ["indels", "strays", "random"])
def test_match_and_gap_at_their_bounds(index, path, kind):
    cols = columns(shape(kind, 300))
    free, _ = check(index, cols, 3, 4, 2, 0)                   # every link is free
    assert (free["score"] == 2 * free["n_words"]).all()
    dear, _ = check(index, cols, 3, 4, 1, 16)                  # nothing but diagonals survives
    assert (dear["pieces"] == 1).all() and not dear["fan_skipped"].any()
    check(index, cols, 3, 63, 16, 16)
    check(index, cols, 1, 63, 16, 1)


# ---- capacity and refusals -------------------------------------------------------------------

def test_capacity_and_refusals_of_the_host_entry_point(path):
    L = _lib.load()
    recs = [(0, 10 + k, 100 + k, 0.0) for k in range(6)] + [(2, 1 + 2 * k, 5 + k, 0.0) for k in range(7)]
    cols = columns(recs)
    want = oracle(cols)
    assert want[0]["n_words"].tolist() == [6, 7]

    def call(cols=cols, n_rows=None, m=6, r=4, s=2, p=1, cap=4, path_cap=20):
        found = np.zeros(max(cap, 1), dtype=abi.ALIGNMENT_DTYPE)
        walk = np.full(max(path_cap, 1), 77, dtype=np.uint32)
        got, got_path = C.c_uint64(99), C.c_uint64(99)
        rc = L.fs_alignments(0, *(abi.ptr(c, t) for c, t in zip(cols, (C.c_uint32,) * 3 + (C.c_double,))),
                             len(cols[0]) if n_rows is None else n_rows, m, r, s, p,
                             found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(got),
                             walk.ctypes.data_as(C.c_void_p) if path_cap else None, path_cap,
                             C.byref(got_path))
        return rc, got.value, got_path.value, found, walk
    rc, n, n_path, found, walk = call()
    assert (rc, n, n_path) == (abi.FS_OK, 2, 13)
    assert_equal((found[:2], walk[:13]), want)
    for cap, path_cap in ((1, 20), (0, 20), (4, 12), (4, 0), (1, 12), (0, 0)):
        rc, n, n_path, found, walk = call(cap=cap, path_cap=path_cap)
        assert (rc, n, n_path) == (abi.FS_E_CAPACITY, 2, 13), (cap, path_cap)
        assert not found["n_words"].any() and (walk == 77).all()
    assert call(cap=2, path_cap=13)[:3] == (abi.FS_OK, 2, 13)
    assert call(m=0)[0] == abi.FS_E_INVALID
    assert call(s=0)[0] == abi.FS_E_INVALID
    assert call(r=64)[0] == abi.FS_E_INVALID
    assert call(s=17)[0] == abi.FS_E_INVALID
    assert call(p=17)[0] == abi.FS_E_INVALID
    assert call(n_rows=1 << 32)[0] == abi.FS_E_UNSUPPORTED
    assert call(n_rows=1 << 28, s=16)[0] == abi.FS_E_UNSUPPORTED
    swapped = [c.copy() for c in cols]
    for c in swapped:
        c[[3, 4]] = c[[4, 3]]
    assert call(cols=swapped)[0] == abi.FS_E_INVALID
    assert b"sorted" in L.fs_last_error()
    assert call(cols=[c[::-1].copy() for c in cols])[0] == abi.FS_E_INVALID
    assert call(cols=(None,) + cols[1:], n_rows=13)[0] == abi.FS_E_INVALID
    assert call(n_rows=0)[:3] == (abi.FS_OK, 0, 0)
    assert call(m=8)[:3] == (abi.FS_OK, 0, 0)                  # nothing kept: no buffer needed
    assert call(m=8, cap=0, path_cap=0)[:3] == (abi.FS_OK, 0, 0)
    rc, n, n_path, found, walk = call()
    ms = (C.c_double * 6)()
    assert L.fs_alignments_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    assert ms[5] >= max(ms[:5])
    empty = alignments.find_alignments(*columns([]))
    assert len(empty[0]) == 0 and len(empty[1]) == 0


def test_capacity_and_refusals_of_the_rows_entry_point(index, path):
    import torch
    from fandom_search_amd.engine import torch_ready
    L = _lib.load()
    recs = [(0, 10 + k, 100 + k, 0.0) for k in range(6)] + [(2, 1 + 2 * k, 5 + k, 0.0) for k in range(7)]
    cols = columns(recs)
    want = oracle(cols)
    d_rows = on_device(cols)
    d_found = torch.zeros(4 * 56, dtype=torch.uint8, device="cuda")
    d_walk = torch.zeros(20, dtype=torch.int32, device="cuda")
    torch_ready()
    ptrs = (d_found.data_ptr(), d_walk.data_ptr())
    for caps in ((1, 20), (4, 12), (0, 0)):
        with pytest.raises(_lib.FsError) as e:
            index.alignments_device(d_rows.data_ptr(), 13, out_ptrs=ptrs, caps=caps)
        assert e.value.code == abi.FS_E_CAPACITY and e.value.required == (2, 13)
        assert not d_found.cpu().numpy().any() and not d_walk.cpu().numpy().any()
    assert index.alignments_device(d_rows.data_ptr(), 13, out_ptrs=ptrs, caps=(2, 13)) == (2, 13)
    assert_equal((d_found.cpu().numpy().view(abi.ALIGNMENT_DTYPE)[:2],
                  d_walk.cpu().numpy().view(np.uint32)[:13]), want)
    ms = (C.c_double * 6)()
    assert L.fs_alignments_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    assert index.alignments_device(d_rows.data_ptr(), 0, out_ptrs=ptrs, caps=(4, 20)) == (0, 0)
    assert L.fs_alignments_times(ms) == abi.FS_OK and not any(ms)
    got, got_path = C.c_uint64(0), C.c_uint64(0)

    def rows_call(rows=d_rows.data_ptr(), n_rows=13, m=6, r=4, s=2, p=1, out=ptrs[0], cap=4,
                  n_out=C.byref(got), to=ptrs[1], path_cap=20, n_path=C.byref(got_path)):
        return L.fs_alignments_rows(index._h, C.c_void_p(rows), n_rows, m, r, s, p, C.c_void_p(out),
                                    cap, n_out, C.c_void_p(to), path_cap, n_path)
    assert rows_call() == abi.FS_OK and (got.value, got_path.value) == (2, 13)
    assert rows_call(m=0) == abi.FS_E_INVALID
    assert rows_call(s=0) == abi.FS_E_INVALID
    assert rows_call(r=64) == abi.FS_E_INVALID
    assert rows_call(s=17) == abi.FS_E_INVALID
    assert rows_call(p=17) == abi.FS_E_INVALID
    assert rows_call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert rows_call(n_rows=1 << 28, s=16) == abi.FS_E_UNSUPPORTED
    assert rows_call(rows=None) == abi.FS_E_INVALID
    assert rows_call(rows=d_rows.data_ptr() + 8) == abi.FS_E_INVALID
    assert rows_call(out=None) == abi.FS_E_INVALID
    assert rows_call(to=None) == abi.FS_E_INVALID
    assert rows_call(n_out=None) == abi.FS_E_INVALID
    assert rows_call(n_path=None) == abi.FS_E_INVALID
    back = torch.cat([d_rows[32 * 12:32 * 13], d_rows[:32 * 12]])   # the last record in front
    torch_ready()
    assert rows_call(rows=back.data_ptr()) == abi.FS_E_INVALID
    assert b"sorted" in L.fs_last_error()


# ---- the command -----------------------------------------------------------------------------

def run_both(tmp_path, source, extra=()):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("a_%s" % reader))
        assert main(["alignments", source, "-o", prefix, "--reader", reader, *extra]) == 0
        got[reader] = tuple(open(name, "rb").read()
                            for name in alignments.output_names(source, prefix))
    assert got["device"] == got["python"]
    return got["device"]


@pytest.mark.parametrize("case,min_words,reach,match,gap", mag.CASES)
def test_golden_cases_under_both_readers(tmp_path, path, case, min_words, reach, match, gap):
    out = run_both(tmp_path, os.path.join(GOLDEN, mag.INPUT),
                   ["--min-words", str(min_words), "--reach", str(reach), "--match", str(match),
                    "--gap", str(gap)])
    for name, part in zip(mag.golden_names(case), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_the_defaults_are_the_default_case(tmp_path):
    out = run_both(tmp_path, os.path.join(GOLDEN, mag.INPUT))
    for name, part in zip(mag.golden_names("default"), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name
