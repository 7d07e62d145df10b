"""`ao3.py matrix --engine device` on the GPU: fs_matrix / fs_matrix_rows against the plain-Python
restatement (tests/matrix_restated.py), the counter, the number of spans and the kept n-grams
compared for equality, every case with the spans sent down each class in turn (FS_MATRIX_SMALL)
and with the hash behind the table of c(v) cut to 4 bits and to nothing (FS_MATRIX_HASH_BITS);
and the command under both engines, byte for byte."""

import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, matrix, synth
from fandom_search_amd.cli import main
from tests import matrix_cases, matrix_restated as mr, util

pytestmark = pytest.mark.gpu

HUGE = str((1 << 32) - 1)
# (FS_MATRIX_SMALL, FS_MATRIX_HASH_BITS): the defaults; every span by a lane; every span by a
# wave; the hash cut to 4 bits and to nothing, the latter also with every span by a wave
MODES = {"default": (None, None), "lane": (HUGE, None), "wave": ("0", None),
         "hash4": (None, "4"), "hash0": (None, "0"), "wave_hash0": ("0", "0")}
NGRAMS = (1, 2, 6, 10)


@pytest.fixture(params=list(MODES), ids=list(MODES))
def mode(request, monkeypatch):
    for name, value in zip(("FS_MATRIX_SMALL", "FS_MATRIX_HASH_BITS"), MODES[request.param]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(500)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def columns(records):
    return tuple(np.asarray([r[k] for r in records], dtype=np.uint32) for k in range(3))


def want_of(records, n, n_script):
    spans, starts, kept = mr.matrix(records, n, n_script)
    return (np.asarray(starts, dtype=np.uint32), len(spans),
            np.array(kept, dtype=abi.MATRIX_NGRAM_DTYPE))


def assert_equal(got, want):
    starts, n_spans, kept = got
    bad = np.flatnonzero(starts != want[0])
    assert not len(bad), (bad[:5], starts[bad[:5]], want[0][bad[:5]])
    assert n_spans == want[1]
    assert kept.dtype == abi.MATRIX_NGRAM_DTYPE and len(kept) == len(want[2])
    for name in kept.dtype.names:
        bad = np.flatnonzero(kept[name] != want[2][name])
        assert not len(bad), (name, bad[:5], kept[name][bad[:5]], want[2][name][bad[:5]])


def check(index, records, n, n_works, n_script, want):
    """fs_matrix and fs_matrix_rows against the restatement's (starts, n_spans, kept)."""
    import torch
    from fandom_search_amd.engine import torch_ready
    cols = columns(records)
    got = matrix.find_ngrams(*cols, n_works, n_script, n)
    assert_equal(got, want)
    rows = np.zeros(len(records), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name] = col
    buf = torch.from_numpy(rows.view(np.uint8).copy()).cuda() if len(rows) else \
        torch.zeros(32, dtype=torch.uint8, device="cuda")
    torch_ready()
    assert_equal(index.matrix_device(buf.data_ptr(), len(rows), n_works, n_script, n), want)
    return got


def numbered(records):
    recs = mr.sort_records(records)
    n_works = max((r[0] for r in recs), default=-1) + 1
    n_script = max((r[2] for r in recs), default=-1) + 1
    return recs, n_works, n_script


# ---- span lengths --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lengths_case(n):
    """A work per span length, the spans overlapping one another in the script."""
    recs = []
    for w, length in enumerate(x for x in (n - 1, n, n + 1, 63, 64, 65, 1023, 1025, 3000) if x):
        recs += [(w, 5 + k, (length * 7) % 50 + k) for k in range(length)]
    recs, n_works, n_script = numbered(recs)
    return recs, n_works, n_script, want_of(recs, n, n_script)


@pytest.mark.parametrize("n", NGRAMS)
def test_span_lengths(index, mode, n):
    recs, n_works, n_script, want = lengths_case(n)
    _, n_spans, kept = check(index, recs, n, n_works, n_script, want)
    assert n_spans == n_works - (1 if n > 1 else 0) and len(kept)


# ---- run heads at lane, wave and workgroup edges -------------------------------------------

@functools.lru_cache(maxsize=None)
def heads_case(n, by_work):
    """Fan runs whose heads lie at records 63, 64, 65, 127 .. 129, 255 .. 257, 511 .. 513: the
    run in front ends by a gap in the fan index, or (by_work) by the next work."""
    recs, fan, at, work = [], 0, 0, 0
    for head in (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 560):
        length = head - at
        recs += [(work, fan + k, (head * 3) % 17 + k) for k in range(length)]
        fan += length + 1
        at = head
        work += 1 if by_work else 0
    recs, n_works, n_script = numbered(recs)
    assert len(mr.fan_runs(recs)) == 13
    return recs, n_works, n_script, want_of(recs, n, n_script)


@pytest.mark.parametrize("by_work", [False, True])
@pytest.mark.parametrize("n", (1, 2))
def test_run_heads_at_edges(index, mode, n, by_work):
    recs, n_works, n_script, want = heads_case(n, by_work)
    check(index, recs, n, n_works, n_script, want)


def test_largest_fan_index(index, mode):
    """0xFFFFFFFE, 0xFFFFFFFF inside a work, then 0 in the next: 0xFFFFFFFF + 1 is not 0."""
    top = (1 << 32) - 1
    recs = [(0, top - 1, 3), (0, top, 4), (1, 0, 5), (1, 1, 6)]
    want = want_of(recs, 2, 8)
    assert want[2].tolist() == [(0, 3), (1, 5)]
    check(index, recs, 2, 2, 8, want)


# ---- repeated and scrambled script words, ties, edges --------------------------------------

@functools.lru_cache(maxsize=None)
def shaped_case(name, n):
    recs, n_works, n_script = numbered(matrix_cases.shaped()[name])
    return recs, n_works, n_script, want_of(recs, n, n_script)


@pytest.mark.parametrize("n", (1, 2, 3, 4))
@pytest.mark.parametrize("name", sorted(matrix_cases.shaped()))
def test_shaped(index, mode, name, n):
    recs, n_works, n_script, want = shaped_case(name, n)
    check(index, recs, n, n_works, n_script, want)


def test_ties(index, mode):
    recs, n_works, n_script, want = shaped_case("tie_inside", 3)
    assert want[2].tolist() == [(0, 10), (1, 10)]              # the first of the equal starts
    recs, n_works, n_script, want = shaped_case("tie_before", 4)
    assert want[1] == 3 and want[2].tolist() == [(0, 10)]      # equal behind: kept; in front: dropped
    check(index, recs, 4, n_works, n_script, want)


@functools.lru_cache(maxsize=None)
def random_case(seed):
    recs, n_works, n_script = numbered(matrix_cases.random_records(seed, n_works=40, n_script=60))
    n = 1 + seed % 4
    return recs, n, n_works, n_script, want_of(recs, n, n_script)


def test_random_files(index, mode):
    kept = 0
    for seed in range(24):
        recs, n, n_works, n_script, want = random_case(seed)
        kept += len(check(index, recs, n, n_works, n_script, want)[2])
    assert kept > 100


@functools.lru_cache(maxsize=None)
def long_run_case(n):
    """One fan run of 700 records whose script words jump: hundreds of spans in a run, ranked
    by a wave; and the same words named twice each."""
    origs = [(k % 350) // 2 * 5 + k % 2 for k in range(700)]
    recs = [(0, k, o) for k, o in enumerate(origs)] + \
        [(1, k, k // 2 * 4 + k % 2) for k in range(600)]
    recs, n_works, n_script = numbered(recs)
    return recs, n_works, n_script, want_of(recs, n, n_script)


@pytest.mark.parametrize("n", (1, 2))
def test_many_spans_in_one_run(index, mode, n):
    recs, n_works, n_script, want = long_run_case(n)
    assert want[1] >= 256
    check(index, recs, n, n_works, n_script, want)


# ---- contention, nothing, errors -----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def contention_case():
    recs = [(w, 3 + k, 2 + k) for w in range(4000) for k in range(8)]
    return recs, want_of(recs, 6, 10)


def test_every_work_quotes_the_same_line(index, mode):
    recs, want = contention_case()
    assert want[0].tolist() == [0, 0, 4000, 4000, 4000, 0, 0, 0, 0, 0]
    assert want[2].tolist() == [(w, 2) for w in range(4000)]
    check(index, recs, 6, 4000, 10, want)


def test_no_span_of_n_words_and_no_records(index, mode):
    recs = [(w, 10 * s + k, 7 * s + k) for w in range(3) for s in range(4) for k in range(5)]
    want = want_of(recs, 6, 40)
    assert want[1] == 0 and not want[0].any()
    check(index, recs, 6, 3, 40, want)
    starts, n_spans, kept = check(index, [], 6, 3, 40, want_of([], 6, 40))
    assert len(starts) == 40 and n_spans == 0 and len(kept) == 0
    check(index, [], 6, 0, 0, want_of([], 6, 0))


def call(cols, n_works, n_script, ngram, cap, n_rows=None, out=True, counts=(True, True)):
    L = _lib.load()
    found = np.zeros(max(1, cap), dtype=abi.MATRIX_NGRAM_DTYPE)
    starts = np.zeros(max(1, min(n_script, 1 << 20)), dtype=np.uint32)
    spans, kept = C.c_uint64(0), C.c_uint64(0)
    ptrs = [abi.ptr(c, C.c_uint32) if c is not None else None for c in cols]
    rc = L.fs_matrix(0, *ptrs, len(cols[1]) if n_rows is None else n_rows, n_works, n_script,
                     ngram, abi.ptr(starts, C.c_uint32),
                     found.ctypes.data_as(C.c_void_p) if out else None, cap,
                     C.byref(spans) if counts[0] else None, C.byref(kept) if counts[1] else None)
    return rc, spans.value, kept.value, found, starts


def test_error_codes_and_capacity():
    recs = [(w, k, 4 + k) for w in range(5) for k in range(6)]
    cols = columns(recs)
    ok = dict(n_works=5, n_script=10, ngram=3, cap=16)
    want = want_of(recs, 3, 10)
    rc, spans, kept, found, starts = call(cols, **ok)
    assert (rc, spans, kept) == (abi.FS_OK, 5, 5)
    assert_equal((starts[:10], spans, found[:kept]), want)
    assert call(cols, **dict(ok, ngram=0))[0] == abi.FS_E_INVALID
    assert call((None, cols[1], cols[2]), **ok)[0] == abi.FS_E_INVALID
    assert call(cols, **ok, out=False)[0] == abi.FS_E_INVALID
    assert call(cols, **ok, counts=(False, True))[0] == abi.FS_E_INVALID
    assert call(cols, **ok, counts=(True, False))[0] == abi.FS_E_INVALID
    assert call(cols, **dict(ok, n_works=4))[0] == abi.FS_E_INVALID          # a work >= n_works
    assert call(cols, **dict(ok, n_script=9))[0] == abi.FS_E_INVALID         # a script index
    assert b"n_script" in _lib.load().fs_last_error()
    back = tuple(c[::-1].copy() for c in cols)
    assert call(back, **ok)[0] == abi.FS_E_INVALID                           # out of order
    assert b"sorted" in _lib.load().fs_last_error()
    assert call(cols, **ok, n_rows=1 << 32)[0] == abi.FS_E_UNSUPPORTED
    assert call(cols, **dict(ok, n_script=abi.FS_WORKS_MAX_SCRIPT + 1))[0] == abi.FS_E_UNSUPPORTED
    assert call(cols, **ok, n_rows=1 << 27)[0] == abi.FS_E_UNSUPPORTED       # tables above 1 GiB
    # the round trip: too small by one says how many, the counter is complete, out untouched
    rc, spans, kept, found, starts = call(cols, **dict(ok, cap=4))
    assert (rc, spans, kept) == (abi.FS_E_CAPACITY, 5, 5)
    assert (starts[:10] == want[0]).all() and not found["start"].any()
    rc, spans, kept, found, starts = call(cols, **dict(ok, cap=5))
    assert rc == abi.FS_OK
    assert_equal((starts[:10], spans, found[:kept]), want)
    # n_rows / ngram + 1 always suffices
    one = [(0, 0, 0)]
    assert call(columns(one), 1, 1, 1, cap=2)[:3] == (abi.FS_OK, 1, 1)
    ms = (C.c_double * 6)()
    assert _lib.load().fs_matrix_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    assert _lib.load().fs_matrix_times(None) == abi.FS_E_INVALID


def test_device_rows_errors_and_capacity(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    recs = [(w, k, 4 + k) for w in range(5) for k in range(6)]
    want = want_of(recs, 3, 10)
    rows = np.zeros(len(recs), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), columns(recs)):
        rows[name] = col
    buf = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    d_starts = torch.zeros(10 * 4, dtype=torch.uint8, device="cuda")
    d_found = torch.zeros(5 * 8, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_starts.data_ptr(), d_found.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        index.matrix_device(buf.data_ptr(), len(rows), 5, 10, 3, out_ptrs=ptrs, cap=4)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == 5
    assert (d_starts.cpu().numpy().view(np.uint32) == want[0]).all()
    assert not d_found.cpu().numpy().any()
    assert index.matrix_device(buf.data_ptr(), len(rows), 5, 10, 3, out_ptrs=ptrs, cap=5) == (5, 5)
    assert (d_found.cpu().numpy().view(abi.MATRIX_NGRAM_DTYPE) == want[2]).all()
    # without the counter
    assert index.matrix_device(buf.data_ptr(), len(rows), 5, 10, 3, out_ptrs=(0, ptrs[1]),
                               cap=5) == (5, 5)
    L = _lib.load()
    spans, kept = C.c_uint64(0), C.c_uint64(0)

    def rows_call(h=index._h, rows=buf.data_ptr(), n_rows=len(rows), n_works=5, n_script=10,
                  ngram=3, out=ptrs[1], cap=5, n_kept=C.byref(kept)):
        return L.fs_matrix_rows(h, C.c_void_p(rows), n_rows, n_works, n_script, ngram,
                                C.c_void_p(ptrs[0]), C.c_void_p(out), cap, C.byref(spans), n_kept)
    assert rows_call() == abi.FS_OK and (spans.value, kept.value) == (5, 5)
    assert rows_call(h=None) == abi.FS_E_INVALID
    assert rows_call(rows=None) == abi.FS_E_INVALID
    assert rows_call(rows=buf.data_ptr() + 8) == abi.FS_E_INVALID
    assert rows_call(out=None) == abi.FS_E_INVALID
    assert rows_call(n_kept=None) == abi.FS_E_INVALID
    assert rows_call(ngram=0) == abi.FS_E_INVALID
    assert rows_call(n_works=4) == abi.FS_E_INVALID
    assert rows_call(n_script=9) == abi.FS_E_INVALID
    assert rows_call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert rows_call(n_script=abi.FS_WORKS_MAX_SCRIPT + 1) == abi.FS_E_UNSUPPORTED


# ---- the command ---------------------------------------------------------------------------

INPUTS = sorted(glob.glob(os.path.join(util.GOLDEN, "matrix_*.in.csv")) +
                glob.glob(os.path.join(util.GOLDEN, "matrix_engine", "*.in.csv")))


def run_both(tmp_path, src, n, tag="m"):
    """{engine: (dense bytes, cells bytes) or the exception's type and text}."""
    got = {}
    for engine in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (tag, engine)))
        try:
            assert main(["matrix", src, prefix, "-n", str(n), "--cells", "--engine", engine]) == 0
        except Exception as e:                       # what the engine raises is compared too
            got[engine] = (type(e), str(e))
            continue
        with open(matrix.matrix_filename(prefix, n), "rb") as fh:
            dense = fh.read()
        with open(matrix.cells_filename(prefix, n), "rb") as fh:
            got[engine] = (dense, fh.read())
    return got


@pytest.mark.parametrize("src", INPUTS, ids=[os.path.basename(p) for p in INPUTS])
def test_command_on_the_committed_inputs(tmp_path, src):
    for n in (1, 3, 4, 6):
        assert matrix.device_tables(src, n) is not None          # the device engine takes it
        got = run_both(tmp_path, src, n, "n%d" % n)
        assert got["device"] == got["python"] and isinstance(got["python"][0], bytes)


@pytest.mark.parametrize("name", sorted(matrix_cases.shaped()))
def test_command_on_repeated_and_scrambled_words(tmp_path, name):
    src = str(tmp_path / "in.csv")
    mr.write_csv(src, matrix_cases.shaped()[name])
    for n in (1, 2, 3):
        assert matrix.device_tables(src, n) is not None
        got = run_both(tmp_path, src, n, "n%d" % n)
        assert got["device"] == got["python"] and isinstance(got["python"][0], bytes)


def test_command_on_files_the_device_engine_hands_over(tmp_path):
    text = open(os.path.join(util.GOLDEN, "matrix_spans_b.in.csv"), newline="").read()
    lines = text.split("\r\n")
    # a batch file: no header row (DictReader takes the first record for one)
    src = str(tmp_path / "batch.csv")
    open(src, "w", newline="").write("\r\n".join(lines[1:]))
    assert matrix.device_tables(src, 4) is None
    got = run_both(tmp_path, src, 4, "batch")
    assert got["device"] == got["python"] and got["python"][0] is KeyError
    # a short row
    src = str(tmp_path / "short.csv")
    open(src, "w", newline="").write("\r\n".join(lines[:3] + ["w1,7,x"] + lines[3:]))
    assert matrix.device_tables(src, 4) is None
    got = run_both(tmp_path, src, 4, "short")
    assert got["device"] == got["python"] and got["python"][0] is TypeError
    # a script word spelt two ways
    src = str(tmp_path / "spelt.csv")
    open(src, "w", newline="").write(text.replace(",W20,", ",w20,", 1))
    assert text.count(",W20,") > 1 and matrix.device_tables(src, 4) is None
    got = run_both(tmp_path, src, 4, "spelt")
    assert got["device"] == got["python"] and isinstance(got["python"][0], bytes)
    # a line break inside a quoted file name: universal newlines turn its '\r\n' into '\n'
    src = str(tmp_path / "crlf.csv")
    open(src, "w", newline="").write(text.replace("w2,", '"w\r\n2",'))
    assert matrix.device_tables(src, 4) is None
    got = run_both(tmp_path, src, 4, "crlf")
    assert got["device"] == got["python"] and b'"w\n2"' in got["python"][0]
    # -n below 1 is the python engine's
    src = os.path.join(util.GOLDEN, "matrix_spans_b.in.csv")
    got = run_both(tmp_path, src, 0, "n0")
    assert got["device"] == got["python"]
