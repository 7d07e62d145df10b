"""`ao3.py retellings` on the GPU: fs_retellings / fs_retellings_rows against the plain-Python
restatement (tests/retellings_restated.py), every field of every fs_retelling and
fs_retelling_passage compared for equality, every case with the works sent down each path in
turn (FS_RETELLINGS_SMALL, FS_RETELLINGS_LDS); and the command under both readers against the
committed expected CSVs."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, retellings, synth
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests import retellings_restated as rt
from tests.golden import make_retellings_golden as mrg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
HUGE = str(1 << 31)
# (FS_RETELLINGS_SMALL, FS_RETELLINGS_LDS): the defaults; every work with a passage through
# global memory; every one through LDS; every one by a single lane
PATHS = {"default": (None, None), "global": ("0", "0"), "lds": ("0", HUGE), "lane": (HUGE, None)}
FAN_GAP = 3                 # fan words between two passages of a work: they never join
P = [1, 2, 8, 9, 63, 64, 65, 128, 129, 300]


@pytest.fixture(params=list(PATHS), ids=list(PATHS))
def path(request, monkeypatch):
    for name, value in zip(("FS_RETELLINGS_SMALL", "FS_RETELLINGS_LDS"), PATHS[request.param]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    return request.param


def layout(works):
    """Columns (work, fan_ix, orig_ix) sorted by (work, fan_ix) of {work: [(orig_first, words),
    ...]}, the passages of a work one behind another."""
    cols = [[], [], []]
    for w in sorted(works):
        fan = 0
        for orig, words in works[w]:
            cols[0] += [w] * words
            cols[1] += range(fan, fan + words)
            cols[2] += range(orig, orig + words)
            fan += words + FAN_GAP
    return tuple(np.asarray(c, dtype=np.uint32) for c in cols)


def oracle(cols, n_works, min_words=6, max_gap=0):
    recs = list(zip(*(c.tolist() for c in cols)))
    works, found = rt.retellings(recs, n_works, min_words, max_gap)
    w = np.array([tuple(r[k] for k in rt.WORK_KEYS) for r in works], dtype=abi.RETELLING_DTYPE)
    p = np.array([tuple(r[k] for k in rt.PASSAGE_KEYS) for r in found],
                 dtype=abi.RETELLING_PASSAGE_DTYPE)
    return w, p


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.RETELLING_DTYPE, abi.RETELLING_PASSAGE_DTYPE)):
        assert a.dtype == dt and len(a) == len(b)
        for name in dt.names:
            bad = np.flatnonzero(a[name] != b[name])
            assert not len(bad), (name, bad[:5], a[name][bad[:5]], b[name][bad[:5]])
    works = got[0]
    has = works["n_passages"] > 0
    assert ((works["n_descents"] == 0) == (works["chain_passages"] == works["n_passages"]))[has].all()
    assert (works["chain_first"][~has] == NONE).all() and not works["chain_words"][~has].any()


def check(cols, n_works, min_words=6, max_gap=0, want=None):
    """fs_retellings against the restatement; returns (works, passages)."""
    got = retellings.find_retellings(*cols, n_works, min_words, max_gap)
    assert_equal(got, oracle(cols, n_works, min_words, max_gap) if want is None else want)
    return got


# ---- one work of p passages ------------------------------------------------------------------

def shape(kind, p):
    """[(orig_first, words)] of p passages; script positions are 50 words apart."""
    if kind == "ascending":
        at, words = list(range(p)), [6] * p
    elif kind == "descending":
        at, words = list(range(p))[::-1], [6] * p
    elif kind == "descending_heavy_middle":
        at, words = list(range(p))[::-1], [6] * p
        words[p // 2] = 9
    elif kind == "sawtooth":
        at, words = [(k % 7) * (p + 1) + k // 7 for k in range(p)], [6 + k % 3 for k in range(p)]
    else:
        rng = np.random.default_rng(p)
        at, words = rng.permutation(p).tolist(), rng.integers(6, 41, p).tolist()
    return [(50 * a, w) for a, w in zip(at, words)]


KINDS = ["ascending", "descending", "descending_heavy_middle", "sawtooth", "random"]


@functools.lru_cache(maxsize=None)
def one_work(kind, p):
    cols = layout({0: shape(kind, p)})
    return cols, oracle(cols, 1)


@pytest.mark.parametrize("p", P)
@pytest.mark.parametrize("kind", KINDS)
def test_one_work_of_p_passages(path, kind, p):
    cols, want = one_work(kind, p)
    works, found = check(cols, 1, want=want)
    assert len(found) == p == works["n_passages"][0]
    if kind == "ascending":
        assert works["chain_passages"][0] == p and works["n_descents"][0] == 0
        assert found["chain_pos"].tolist() == list(range(1, p + 1))
    if kind == "descending":
        assert works["chain_passages"][0] == 1 and works["chain_last"][0] == 0
        assert works["n_descents"][0] == p - 1
    if kind == "descending_heavy_middle":
        assert works["chain_last"][0] == p // 2 and works["chain_words"][0] == 9


def test_zero_records_one_record_one_passage(path):
    none = (np.zeros(0, dtype=np.uint32),) * 3
    works, found = check(none, 3)
    assert len(found) == 0 and works.tolist() == [(0, 0, 0, 0, NONE, NONE, 0, 0, 0, 0)] * 3
    assert len(check(none, 0)[0]) == 0
    one = tuple(np.asarray([v], dtype=np.uint32) for v in (4, 9, 2))
    works, found = check(one, 6, min_words=1)
    assert found.tolist() == [(0, 1, 4, 9, 9, 2, 2, 1, NONE, 1, 1)]
    assert works[4].tolist() == (1, 1, 1, 1, 0, 0, 2, 2, 1, 0)
    assert len(check(one, 6, min_words=2)[1]) == 0
    works, found = check(layout({0: [(10, 6)]}), 1)
    assert found.tolist() == [(0, 6, 0, 0, 5, 10, 15, 6, NONE, 1, 1)]


# ---- ties and strictness ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 64, 70, 200])
def test_many_equal_candidates_for_one_later_passage(path, k):
    spans = [(50 * (k - j), 6) for j in range(k)] + [(50 * (k + 5), 6)]
    works, found = check(layout({0: spans}), 1)
    assert found["prev"][k] == 0 and found["best"][k] == 12 and works["chain_first"][0] == 0


def test_two_ends_with_equal_best(path):
    works, found = check(layout({0: [(100, 6), (50, 6), (110, 6), (60, 6)]}), 1)
    assert found["prev"].tolist() == [NONE, NONE, 0, 1]
    assert (works["chain_first"][0], works["chain_last"][0]) == (0, 2)
    assert found["chain_pos"].tolist() == [1, 0, 2, 0]


@pytest.mark.parametrize("lead", [63, 127])
def test_a_plateau_across_a_64_boundary(path, lead):
    # passages 0 .. lead-1 lie too late in the script to be followed; passages `lead` and
    # lead + 1 (the last of a tile and the first of the next) tie for the passage behind them
    spans = [(100_000 - 50 * j, 6) for j in range(lead)] + [(500, 6), (400, 6), (600, 6), (700, 7)]
    works, found = check(layout({0: spans}), 1)
    assert found["best"][lead:].tolist() == [6, 6, 12, 19]
    assert found["prev"][lead:].tolist() == [NONE, NONE, lead, lead + 2]
    assert (works["chain_first"][0], works["chain_last"][0]) == (lead, lead + 3)
    # a plateau of equal best: every end ties, the first passage wins
    flat = [(100_000 - 50 * j, 6) for j in range(lead + 3)]
    works, found = check(layout({0: flat}), 1)
    assert works["chain_last"][0] == 0 and (found["best"] == 6).all()


@pytest.mark.parametrize("step", [-1, 0, 1])
def test_strictness(path, step):
    works, found = check(layout({0: [(10, 6), (15 + step, 6)]}), 1)
    assert works["chain_passages"][0] == (2 if step == 1 else 1)
    assert works["n_descents"][0] == (0 if step == 1 else 1)


def test_max_gap_and_a_repeated_fan_index(path):
    recs = ([(0, f, 100 + f) for f in (0, 1, 2, 4, 5, 6)]           # one word bridged
            + [(0, 20 + f, 200 + f) for f in (0, 1, 2, 5, 6, 7)]    # two words bridged
            + [(0, 40 + f, 300 + f) for f in range(4)] + [(0, 43, 304), (0, 44, 305), (0, 45, 306)]
            + [(1, f, 50 + 2 * f) for f in range(5)]                # the script steps 2, the fan 1
            + [(1, 10 + f, 10 + f) for f in range(3)])
    cols = tuple(np.asarray(c, dtype=np.uint32) for c in zip(*recs))
    for gap, counts in ((0, [6, 1]), (1, [5, 2]), (2, [4, 2])):
        works, found = check(cols, 2, min_words=3, max_gap=gap)
        assert works["n_passages"].tolist() == counts
    works, found = check(cols, 2, min_words=3, max_gap=1)
    assert found["n_words"].tolist() == [6, 3, 3, 4, 3, 5, 3]
    assert found["orig_last"][0] == 106 and found["first"][3] == 12 and found["first"][4] == 16


# ---- many works ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(7)
    n_works = 460
    ids = rng.permutation(n_works).tolist()
    sizes = [int(rng.integers(1, 4)) for _ in range(400)] + \
        [int(rng.integers(10, 71)) for _ in range(20)] + [300, 300]
    order = rng.permutation(len(sizes)).tolist()                    # the classes interleaved
    works = {}
    for k in order:
        p = sizes[k]
        at = rng.permutation(4 * p)[:p] if k % 3 else np.sort(rng.permutation(4 * p)[:p])
        works[ids.pop()] = [(50 * int(a), int(rng.integers(6, 41))) for a in at]
    short = [ids.pop() for _ in range(20)]                          # runs below min_words only
    for w in short:
        works[w] = [(50 * j, 5) for j in range(3)]
    assert len(ids) == 18                                           # works without records
    cols = layout(works)
    return cols, n_works, oracle(cols, n_works), short + ids


def test_works_of_every_class_in_one_input(path):
    cols, n_works, want, empty = mixed()
    works, found = check(cols, n_works, want=want)
    assert sorted(np.flatnonzero(works["n_passages"] == 0).tolist()) == sorted(empty)
    assert (works["n_passages"] == 300).sum() == 2 and (works["n_passages"] <= 3).sum() >= 400
    assert [tuple(w) for w in works[empty].tolist()] == [(0, 0, 0, 0, NONE, NONE, 0, 0, 0, 0)] * 38


# fs_retellings.hip: k_rt_kept counts the kept runs of 256 runs, and the one-workgroup scan
# takes 1024 such counts per chunk
RUN_CHUNK = 1024 * 256


@pytest.mark.parametrize("n", [RUN_CHUNK - 1, RUN_CHUNK + 1])
def test_kept_runs_around_the_scan_s_chunk(monkeypatch, n):
    """Every record its own kept run (the fan index steps by 2), four to a work: one run short
    of a chunk of the scan of the kept-run counts, and one run into its second chunk."""
    for name in ("FS_RETELLINGS_SMALL", "FS_RETELLINGS_LDS"):
        monkeypatch.delenv(name, raising=False)
    i = np.arange(n, dtype=np.int64)
    orig = np.random.default_rng(n).integers(0, 997, n)
    cols = tuple(np.asarray(c, dtype=np.uint32) for c in (i // 4, 2 * (i % 4), orig))
    n_works = (n + 3) // 4
    works, found = check(cols, n_works, min_words=1)
    assert len(found) == n and found["first"].tolist() == list(range(n))
    assert works["n_passages"].tolist() == [4] * (n // 4) + [n % 4] * (n_works - n // 4)
    assert 2 < works["chain_passages"].mean() < 3


# ---- capacity and refusals -------------------------------------------------------------------

def call(cols, n_works, min_words, max_gap, cap, n_rows=None, out=True):
    L = _lib.load()
    works = np.full(max(n_works, 1), 7, dtype=np.uint32).repeat(10).view(abi.RETELLING_DTYPE)
    found = np.zeros(max(cap, 1), dtype=abi.RETELLING_PASSAGE_DTYPE)
    got = C.c_uint64(99)
    rc = L.fs_retellings(0, *(abi.ptr(c, C.c_uint32) for c in cols),
                         len(cols[0]) if n_rows is None else n_rows, n_works, min_words, max_gap,
                         works.ctypes.data_as(C.c_void_p) if out else None,
                         found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(got))
    return rc, got.value, works[:n_works], found


def test_capacity_and_refusals(path):
    cols = layout({0: [(10, 6), (30, 6)], 2: [(40, 7), (20, 6), (60, 6)]})
    want_w, want_p = oracle(cols, 3)
    assert len(want_p) == 5
    for cap in (0, 4, 5, 9):
        rc, n, works, found = call(cols, 3, 6, 0, cap)
        assert rc == (abi.FS_OK if cap >= 5 else abi.FS_E_CAPACITY) and n == 5
        assert_equal((works, found[:5] if cap >= 5 else want_p), (want_w, want_p))   # out is complete
        if cap < 5:
            assert not found["n_words"].any()
    ok = dict(n_works=3, min_words=6, max_gap=0, cap=9)
    assert call(cols, **dict(ok, n_works=2))[0] == abi.FS_E_INVALID
    assert b"n_works" in _lib.load().fs_last_error()
    assert call(cols, **dict(ok, n_works=0), out=False)[0] == abi.FS_E_INVALID
    assert call(cols, **dict(ok, min_words=0))[0] == abi.FS_E_INVALID
    assert call(cols, **ok, out=False)[0] == abi.FS_E_INVALID
    assert call((None, cols[1], cols[2]), **ok, n_rows=len(cols[0]))[0] == abi.FS_E_INVALID
    swapped = [c.copy() for c in cols]
    for c in swapped:
        c[[3, 4]] = c[[4, 3]]
    assert call(swapped, **ok)[0] == abi.FS_E_INVALID
    assert b"sorted" in _lib.load().fs_last_error()
    assert call([c[::-1].copy() for c in cols], **ok)[0] == abi.FS_E_INVALID
    assert call(cols, **ok, n_rows=1 << 32)[0] == abi.FS_E_UNSUPPORTED
    rc, n, works, found = call(cols, **ok)
    assert rc == abi.FS_OK and n == 5
    ms = (C.c_double * 6)()
    assert _lib.load().fs_retellings_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    assert ms[5] >= max(ms[:5])


# ---- device rows after a search --------------------------------------------------------------

def test_device_rows_after_a_search(synth_base, path):
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    vocab, emb = synth_base["words"], synth_base["emb"]
    n_works, per, n = 300, 2000, 6
    script = synth.script_tokens(5000)
    tok, off = synth.corpus_tokens(n_works, per, script)
    ix = ScriptIndex(script, [vocab[int(t)] for t in script], emb, synth.lsh_normals(n))
    corpus = ix.corpus(tok, off, synth_base["chars"], synth_base["off"])
    cap = len(tok) // 4
    buf = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    n_rows, _ = ix.search_device(corpus, buf.data_ptr(), cap)
    rows = buf[:n_rows * 32].cpu().numpy().view(abi.ROW_DTYPE)
    cols = tuple(np.ascontiguousarray(rows[c]) for c in ("work", "fan_ix", "orig_ix"))
    for g in (0, 1):
        dev = ix.retellings_device(buf.data_ptr(), n_rows, n_works, n, g)
        host = retellings.find_retellings(*cols, n_works, n, g)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, n, g))
        if g == 0:
            first = dev
    works, found = first
    k = len(found)
    assert k >= 10 and (works["n_passages"] > 1).any()
    # the caller's own device buffers, the passages' too small by one first
    d_works = torch.zeros(n_works * 40, dtype=torch.uint8, device="cuda")
    d_found = torch.zeros(k * 48, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_works.data_ptr(), d_found.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        ix.retellings_device(buf.data_ptr(), n_rows, n_works, n, 0, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_works.cpu().numpy().view(abi.RETELLING_DTYPE) == works).all()
    assert not d_found.cpu().numpy().any()
    assert ix.retellings_device(buf.data_ptr(), n_rows, n_works, n, 0, out_ptrs=ptrs, cap=k) == k
    assert (d_found.cpu().numpy().view(abi.RETELLING_PASSAGE_DTYPE) == found).all()
    ms = (C.c_double * 6)()
    assert _lib.load().fs_retellings_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    # no records: works without a passage on the device
    assert ix.retellings_device(buf.data_ptr(), 0, n_works, n, out_ptrs=ptrs, cap=k) == 0
    none = d_works.cpu().numpy().view(abi.RETELLING_DTYPE)
    assert (none["chain_first"] == NONE).all() and not none["n_passages"].any()
    # the rules of the host entry point
    L = _lib.load()
    got = C.c_uint64(0)

    def rows_call(n_rows=n_rows, n_works=n_works, min_words=n, rows=buf.data_ptr(), out=ptrs[0],
                  passages=ptrs[1], cap=k, n_out=C.byref(got)):
        return L.fs_retellings_rows(ix._h, C.c_void_p(rows), n_rows, n_works, min_words, 0,
                                    C.c_void_p(out), C.c_void_p(passages), cap, n_out)
    assert rows_call() == abi.FS_OK and got.value == k
    assert rows_call(min_words=0) == abi.FS_E_INVALID
    assert rows_call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert rows_call(rows=None) == abi.FS_E_INVALID
    assert rows_call(out=None) == abi.FS_E_INVALID
    assert rows_call(passages=None) == abi.FS_E_INVALID
    assert rows_call(n_out=None) == abi.FS_E_INVALID
    assert rows_call(n_works=int(cols[0].max())) == abi.FS_E_INVALID
    assert rows_call(rows=buf.data_ptr() + 32 * (n_rows - 1), n_rows=1) == abi.FS_OK
    # records out of order: the last record in front of the first
    back = torch.cat([buf[32 * (n_rows - 1):32 * n_rows], buf[:32 * (n_rows - 1)]])
    torch_ready()
    assert rows_call(rows=back.data_ptr()) == abi.FS_E_INVALID


# ---- the command -----------------------------------------------------------------------------

def run_both(tmp_path, path, extra=(), tag="r"):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (tag, reader)))
        assert main(["retellings", path, "-o", prefix, "--reader", reader, *extra]) == 0
        got[reader] = tuple(open(name, "rb").read()
                            for name in retellings.output_names(path, prefix))
    assert got["device"] == got["python"]
    return got["device"]


def options(min_words, max_gap, min_passages, min_share):
    return ["--min-words", str(min_words), "--max-gap", str(max_gap), "--min-passages",
            str(min_passages), "--min-share", str(min_share)]


@pytest.mark.parametrize("case,min_words,max_gap,min_passages,min_share", mrg.CASES)
def test_golden_cases_under_both_readers(tmp_path, path, case, min_words, max_gap, min_passages,
                                         min_share):
    out = run_both(tmp_path, os.path.join(GOLDEN, mrg.INPUT),
                   options(min_words, max_gap, min_passages, min_share))
    for name, part in zip(mrg.golden_names(case), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_the_defaults_are_the_default_case(tmp_path):
    out = run_both(tmp_path, os.path.join(GOLDEN, mrg.INPUT))
    for name, part in zip(mrg.golden_names("default"), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_an_off_grammar_file_gives_the_python_reader_s_output(tmp_path):
    with open(os.path.join(GOLDEN, mrg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    parts = lines[5].split(b",")
    parts[2] = b'fee"l"in'                       # a quote inside a field: csv.reader takes it
    lines[5] = b",".join(parts)
    path = tmp_path / "m.csv"
    path.write_bytes(b"\r\n".join(lines))
    with MatchFile(str(path)) as mf:
        assert mf.outside and mf.reason & abi.FS_MATCH_BAD_OPEN
    out = run_both(tmp_path, str(path), options(6, 0, 1, 0))
    assert b'fee""l""in' in out[1]
    assert out == tuple(p.encode("utf-8") for p in
                        rt.retellings_csv(path.read_bytes().decode("utf-8"), 6, 0, 1, 0))


def test_two_labels_for_one_script_word(tmp_path):
    with open(os.path.join(GOLDEN, mrg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    parts = lines[40].split(b",")
    parts[-4] = b"99"                             # the same script word in another scene
    lines[40] = b",".join(parts)
    path = tmp_path / "m.csv"
    path.write_bytes(b"\r\n".join(lines))
    errs = []
    for reader in ("device", "python"):
        with pytest.raises(SystemExit) as e:
            main(["retellings", str(path), "-o", str(tmp_path / "o"), "--reader", reader])
        errs.append(str(e.value.code))
    assert errs[0] == errs[1]
    assert errs[0].startswith("ao3.py retellings: error: script word ") and "two scenes" in errs[0]
