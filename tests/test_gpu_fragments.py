"""`fragments` on the GPU: fs_fragments and fs_fragments_rows against the restated contract
(tests/fragments_restated.py), every field of every fragment and work compared for equality,
the reserved word too, down every spread path (the dedupe, the plain per-run spread, the
dedupe with its hash cut); run lengths and positions around the 64-bit words of the coverage,
the flags at their edges, numbers of active works around a tile, contention on one cell; the
counts of fs_lines, fs_quotes and fs_pairs on the same records; `ao3.py fragments` byte for
byte against the committed files."""

import ctypes as C
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, fragments, lines, pairs, quotes, synth
from fandom_search_amd.cli import main
from fandom_search_amd.command import grow
from tests import fragments_restated as fr
from tests import pairs_restated as plr
from tests.golden import make_fragments_golden as mfg
from tests.test_gpu_lines import random_works
from tests.test_gpu_pairs import from_spans, interleaved

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE
N_SCRIPT = 3000          # of the index behind fs_fragments_rows; every case uses it
DTYPES = (abi.FRAGMENT_DTYPE, abi.FRAGMENT_WORK_DTYPE)
LENGTHS = (1, 2, 63, 64, 65, 128, 129)
# the spread paths: the dedupe, every run by itself, the dedupe with 2 bits and with no bit of
# its hash
PATHS = ({}, {"FS_FRAGMENTS_DEDUP": "0"}, {"FS_FRAGMENTS_HASH_BITS": "2"},
         {"FS_FRAGMENTS_HASH_BITS": "0"})


@pytest.fixture(scope="module")
def index(synth_base):
    from fandom_search_amd.engine import ScriptIndex
    script = synth.script_tokens(N_SCRIPT)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    yield ix
    ix.close()


def oracle(cols, n_works, m, g, k, lo, hi):
    recs = list(zip(*(c.tolist() for c in cols)))
    parts = fr.fragments(recs, n_works, N_SCRIPT, m, g, k, lo, hi)
    out = []
    for part, keys, dt in zip(parts, (fr.FRAGMENT_KEYS, fr.WORK_KEYS), DTYPES):
        a = np.zeros(len(part), dtype=dt)                  # (the reserved word: 0)
        for name in keys:
            a[name] = [d[name] for d in part]
        out.append(a)
    return tuple(out)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def on_device(cols):
    import torch
    rows = np.zeros(max(1, len(cols[0])), dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix"), cols):
        rows[name][:len(col)] = col
    return torch.from_numpy(rows.view(np.uint8)).to("cuda")


def check(index, monkeypatch, cols, n_works, m=3, g=0, k=2, lo=3, hi=128, paths=PATHS,
          some=True):
    """Both entry points down every path of `paths` against the oracle, which lists a fragment
    unless the case is meant to have none; the oracle's result."""
    from fandom_search_amd.engine import torch_ready
    want = oracle(cols, n_works, m, g, k, lo, hi)
    assert not some or len(want[0])
    d_rows = on_device(cols)
    torch_ready()
    for env in paths:
        for name in ("FS_FRAGMENTS_DEDUP", "FS_FRAGMENTS_HASH_BITS"):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        got = fragments.find_fragments(*cols, n_works, N_SCRIPT, m, g, k, lo, hi)
        assert_equal(got, want)
        dev = index.fragments_device(d_rows.data_ptr(), len(cols[0]), n_works, m, g, k, lo, hi)
        assert_equal(dev, want)
    for name in ("FS_FRAGMENTS_DEDUP", "FS_FRAGMENTS_HASH_BITS"):
        monkeypatch.delenv(name, raising=False)
    return want


# ---- run lengths and where a run starts in a coverage word ---------------------------------

def placed(bit):
    """(start, words) of a run of every length of LENGTHS, each starting at bit `bit` of a
    64-bit word of the coverage, two uncovered words at least between them."""
    out, at = [], 0
    for n in LENGTHS:
        start = at + (bit - at) % 64
        out.append((start, n))
        at = start + n + 2
    assert at < N_SCRIPT - 10
    return out


@pytest.mark.parametrize("bit", [0, 1, 62, 63])
def test_run_lengths_at_every_place_of_a_coverage_word(index, monkeypatch, bit):
    spans_of = []
    for a, n in placed(bit):
        spans_of += [[(a, n)], [(a, n)]]                               # the run, twice
        if n >= 3:
            spans_of.append([(a + 1, n - 2)])                          # neither end
        if n >= 2:
            spans_of.append([(a, n // 2)])                             # its start only
            spans_of.append([(a + n // 2, n - n // 2)])                # its end only
    spans_of += [[(N_SCRIPT - 5, 5)], [(N_SCRIPT - 9, 9)]]             # to the script's last word
    spans_of.append([(0, N_SCRIPT)])                                   # a run of every word
    cols = from_spans(spans_of)
    crossed = [(a >> 6, (a + n - 1) >> 6) for a, n in placed(bit)]
    assert any(k1 - k0 == 1 for k0, k1 in crossed) and any(k1 - k0 >= 2 for k0, k1 in crossed)
    found, works = check(index, monkeypatch, cols, len(spans_of), m=1, k=2, lo=1, hi=128)
    listed = set(zip(found["first"].tolist(), found["last"].tolist()))
    for a, n in placed(bit):
        assert ((a, a + n - 1) in listed) == (n <= 128), (a, n)
    assert (N_SCRIPT - 5, N_SCRIPT - 1) in listed and (N_SCRIPT - 9, N_SCRIPT - 1) in listed
    assert works["runs"].tolist() == [1] * len(spans_of)
    assert works["longest_works"][-1] == NONE and works["covered"][-1] == N_SCRIPT
    # every length listed: the longest row is the run of 129 words
    found, _ = check(index, monkeypatch, cols, len(spans_of), m=1, k=2, lo=1, hi=129,
                     paths=PATHS[:2])
    assert (found["last"] - found["first"]).max() == 128
    # and a random cover under passages of three and more words
    cols, n_works = random_works(40, seed=bit, hi=250, most=5)
    check(index, monkeypatch, cols, n_works, m=3, k=2, lo=3, hi=128, paths=PATHS[:2])


def test_abutting_and_overlapping_passages_of_one_work_make_one_run(index, monkeypatch):
    # work 0: two passages that abut, work 1: two that overlap, work 2: the stretch in one
    cols = from_spans([[(100, 6), (106, 6)], [(100, 8), (104, 8)], [(100, 12)], [(300, 4)]])
    found, works = check(index, monkeypatch, cols, 4, m=3, k=3, lo=3, hi=128)
    assert found.tolist() == [(100, 111, 3, 3, 3, 3, 0, 0)]            # no passage alone holds it
    assert works["runs"].tolist() == [1, 1, 1, 1] and works["held"].tolist() == [1, 1, 1, 0]
    assert works["exact"].tolist() == [1, 1, 1, 0]


# ---- the flags at their edges --------------------------------------------------------------

def test_max_words_min_length_and_min_works_at_their_edges(index, monkeypatch):
    # [100, 109] by works 0 and 1, [100, 120] by work 2, [103, 105] by work 3
    cols = from_spans([[(100, 10)], [(100, 10)], [(100, 21)], [(103, 3)]])
    two = PATHS[:2]
    for hi, there in ((10, True), (9, False), (11, True)):
        found, _ = check(index, monkeypatch, cols, 4, m=3, k=2, lo=3, hi=hi, paths=two)
        assert ((found["first"] == 100) & (found["last"] == 109)).any() == there
    found, works = check(index, monkeypatch, cols, 4, m=3, k=1, lo=1, hi=21, paths=two)
    assert found[["first", "last", "works"]].tolist() == [(103, 105, 4), (100, 109, 3),
                                                          (100, 120, 1)]
    assert works["longest_works"].tolist() == [3, 3, 1, 4]
    found, works = check(index, monkeypatch, cols, 4, m=3, k=1, lo=10, hi=10, paths=two)
    assert found[["first", "last"]].tolist() == [(100, 109)]           # min_length = max_words
    assert works["longest_works"].tolist() == [3, 3, NONE, NONE]
    # exactly at a cell's support, and one above it
    found, _ = check(index, monkeypatch, cols, 4, m=3, k=3, lo=3, hi=128, paths=two)
    assert found[["first", "last", "works"]].tolist() == [(103, 105, 4), (100, 109, 3)]
    found, _ = check(index, monkeypatch, cols, 4, m=3, k=4, lo=3, hi=128, paths=two)
    assert found[["first", "last", "works"]].tolist() == [(103, 105, 4)]
    check(index, monkeypatch, cols, 4, m=3, k=5, lo=3, hi=128, paths=two, some=False)


# ---- active works: the edges of a tile of 64 ----------------------------------------------

@pytest.mark.parametrize("n_active", [1, 63, 64, 65, 129])
def test_active_works_around_a_tile(index, monkeypatch, n_active):
    cols, n_works = random_works(n_active, seed=n_active, lo=3, hi=60, most=4)
    assert n_works > n_active                              # active numbers are not work numbers
    k = 1 if n_active == 1 else 2
    found, works = check(index, monkeypatch, cols, n_works, m=3, k=k, lo=3, hi=128,
                         paths=PATHS[:2])
    assert len(works) == n_active
    assert (np.diff(works["work"].astype(np.int64)) > 0).all()
    assert works["held"].sum() == found["works"].sum()


# ---- contention ----------------------------------------------------------------------------

def test_three_hundred_works_on_one_run_on_one_start_and_on_one_end(index, monkeypatch):
    def spans(k, rng):
        return [(500, 12), (700, 3 + k % 50), (960 - (3 + k % 37), 3 + k % 37)]
    spans_of = interleaved(300, spans, seed=3)
    found, works = check(index, monkeypatch, from_spans(spans_of), len(spans_of), m=3, k=2,
                         lo=3, hi=128)
    first_active = next(w for w, s in enumerate(spans_of) if len(s) == 3)
    same = found[(found["first"] == 500) & (found["last"] == 511)]
    assert same.tolist() == [(500, 511, 300, 300, 300, 300, first_active, 0)]
    starts = found[found["first"] == 700]
    assert len(starts) == 50 and starts["works"].max() == 300 and starts["works"].min() == 6
    assert (starts["start_works"] == starts["works"]).all()
    ends = found[found["last"] == 959]
    assert len(ends) == 37 and (ends["end_works"] == ends["works"]).all()
    assert (works["runs"] == 3).all() and len(works) == 300


# ---- random works ----------------------------------------------------------------------------

def open_cells(cols, n_works, m, k, lo, hi):
    """(cells with S >= k that a word more on the left keeps whole and one on the right does
    not, the same with the sides exchanged), from the coverage sets."""
    recs = list(zip(*(c.tolist() for c in cols)))
    sup = fr.Support(plr.coverage(recs, n_works, m, 0), N_SCRIPT)
    left, right = [], []
    for a in range(N_SCRIPT):
        for n in range(lo, min(hi, sup.longest_from(a)) + 1):
            b = a + n - 1
            s = sup.S(a, b)
            if s < k:
                continue
            more_left, more_right = sup.S(a - 1, b) == s, sup.S(a, b + 1) == s
            if more_left and not more_right:
                left.append((a, b))
            if more_right and not more_left:
                right.append((a, b))
    return left, right


@pytest.mark.parametrize("seed", [11, 12])
def test_random_works_with_listed_and_half_open_cells(index, monkeypatch, seed):
    cols, n_works = random_works(90, seed=seed, lo=3, hi=120, most=5)
    left, right = open_cells(cols, n_works, 3, 2, 3, 128)
    assert left and right
    found, works = check(index, monkeypatch, cols, n_works, m=3, k=2, lo=3, hi=128)
    listed = set(zip(found["first"].tolist(), found["last"].tolist()))
    assert len(listed) > 20 and not listed & set(left) and not listed & set(right)
    assert works["held"].sum() == found["works"].sum()
    check(index, monkeypatch, cols, n_works, m=3, g=1, k=3, lo=5, hi=40, paths=PATHS[:2])
    L = _lib.load()
    ms = (C.c_double * 5)()
    assert L.fs_fragments_times(ms) == abi.FS_OK and min(ms[0:4]) > 0
    assert abs(ms[4] - sum(ms[0:4])) < 1e-9


def test_every_run_is_a_fragment_under_the_loosest_flags(index, monkeypatch):
    cols, n_works = random_works(50, seed=21, lo=3, hi=90, most=4)
    found, works = check(index, monkeypatch, cols, n_works, m=3, k=1, lo=1, hi=400,
                         paths=PATHS[:2])
    assert (works["exact"] == works["runs"]).all() and works["runs"].sum() > 100
    assert found["exact_works"].sum() == works["runs"].sum()


# ---- capacities, refusals and edges --------------------------------------------------------

def _call(L, cols, n_works, frags, f_cap, n_frags, works, w_cap, n_active, m=3, k=2, lo=3,
          hi=128, n_rows=None, n_script=N_SCRIPT):
    return L.fs_fragments(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                          abi.ptr(cols[2], C.c_uint32), len(cols[0]) if n_rows is None else n_rows,
                          n_works, n_script, m, 0, k, lo, hi,
                          frags.ctypes.data_as(C.c_void_p) if f_cap else None, f_cap,
                          C.byref(n_frags),
                          works.ctypes.data_as(C.c_void_p) if w_cap else None, w_cap,
                          C.byref(n_active))


def test_capacities_too_small_exact_and_grown_from_one(index):
    import torch
    from fandom_search_amd.engine import torch_ready
    cols, n_works = random_works(100, seed=8, hi=60)
    cols = [np.ascontiguousarray(c) for c in cols]
    want = oracle(cols, n_works, 3, 0, 2, 3, 128)
    nf, na = len(want[0]), len(want[1])
    assert na == 100 and nf > 20
    L = _lib.load()
    frags = np.zeros(nf, dtype=abi.FRAGMENT_DTYPE)
    works = np.zeros(na, dtype=abi.FRAGMENT_WORK_DTYPE)
    n_frags, n_active = C.c_uint64(0), C.c_uint64(0)
    for f_cap, w_cap in ((nf, 0), (nf, na - 1), (nf - 1, na), (0, 0)):
        rc = _call(L, cols, n_works, frags, f_cap, n_frags, works, w_cap, n_active)
        assert rc == abi.FS_E_CAPACITY and (n_frags.value, n_active.value) == (nf, na)
        assert not frags["works"].any() and not works["runs"].any()    # both untouched
    assert _call(L, cols, n_works, frags, nf, n_frags, works, na, n_active) == abi.FS_OK
    assert (n_frags.value, n_active.value) == (nf, na)
    assert_equal((frags, works), want)
    # both buffers grow from room for one record
    rows = [abi.ptr(c, C.c_uint32) for c in cols]
    grown = grow(lambda f_out, f_cap, f_got, w_out, w_cap, w_got: L.fs_fragments(
        0, rows[0], rows[1], rows[2], len(cols[0]), n_works, N_SCRIPT, 3, 0, 2, 3, 128, f_out,
        f_cap, f_got, w_out, w_cap, w_got), list(DTYPES), [1, 1], "fs_fragments")
    assert_equal(grown, want)
    d_rows = on_device(cols)
    torch_ready()
    args = (d_rows.data_ptr(), len(cols[0]), n_works, 3, 0, 2, 3, 128)
    assert_equal(index.fragments_device(*args, caps=(1, 1)), want)
    # the caller's own device buffers
    d_frags = torch.zeros(nf * 32, dtype=torch.uint8, device="cuda")
    d_works = torch.zeros(na * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_frags.data_ptr(), d_works.data_ptr())
    for caps in ((nf, na - 1), (nf - 1, na), (0, na)):
        with pytest.raises(_lib.FsError) as e:
            index.fragments_device(*args, out_ptrs=ptrs, caps=caps)
        assert e.value.code == abi.FS_E_CAPACITY and e.value.required == (nf, na)
        assert not d_frags.cpu().numpy().any() and not d_works.cpu().numpy().any()
    assert index.fragments_device(*args, out_ptrs=ptrs, caps=(nf, na)) == (nf, na)
    assert (d_frags.cpu().numpy().view(abi.FRAGMENT_DTYPE) == want[0]).all()
    assert (d_works.cpu().numpy().view(abi.FRAGMENT_WORK_DTYPE) == want[1]).all()
    # no records on the device
    assert index.fragments_device(d_rows.data_ptr(), 0, n_works, 3, 0, 2, 3, 128, out_ptrs=ptrs,
                                  caps=(nf, na)) == (0, 0)


def test_no_records_no_passage_and_a_min_length_beyond_the_script(index, monkeypatch):
    empty = (np.zeros(0, np.uint32),) * 3
    found, works = check(index, monkeypatch, empty, 3, some=False)
    assert len(found) == 0 and len(works) == 0
    cols, n_works = random_works(10, seed=2)
    found, works = check(index, monkeypatch, cols, n_works, m=41, some=False)
    assert len(found) == 0 and len(works) == 0
    whole = from_spans([[(0, N_SCRIPT)], [(0, N_SCRIPT)]])
    found, works = check(index, monkeypatch, whole, 2, lo=N_SCRIPT, hi=4096)   # one row, one cell
    assert found.tolist() == [(0, N_SCRIPT - 1, 2, 2, 2, 2, 0, 0)]
    assert works.tolist() == [(w, 1, N_SCRIPT, 1, 1, 0, N_SCRIPT - 1, 2) for w in (0, 1)]
    found, works = check(index, monkeypatch, whole, 2, lo=4000, hi=4096, some=False)
    assert works.tolist() == [(w, 1, N_SCRIPT, 0, 0, 0, N_SCRIPT - 1, NONE) for w in (0, 1)]


def test_refusals(index, monkeypatch):
    from fandom_search_amd.engine import torch_ready
    from tests.test_gpu_pairs import records
    cols = records([300, 500, 200], N_SCRIPT, seed=9)

    def refused(c, n_works=3, m=6, lo=3, hi=128, code=abi.FS_E_INVALID, n_script=N_SCRIPT,
                rows=True, says=None):
        with pytest.raises(_lib.FsError) as e:
            fragments.find_fragments(*c, n_works, n_script, m, 0, 2, lo, hi)
        assert e.value.code == code and (says is None or says in str(e.value))
        if rows:
            d_rows = on_device(c)
            torch_ready()
            with pytest.raises(_lib.FsError) as e:
                index.fragments_device(d_rows.data_ptr(), len(c[0]), n_works, m, 0, 2, lo, hi)
            assert e.value.code == code
    refused(cols, m=0)
    refused(cols, lo=0)                                    # min_length == 0
    refused(cols, lo=4, hi=3)                              # max_words < min_length
    refused(cols, n_works=2)                               # a work >= n_works
    far = cols[2].copy()
    far[20] = N_SCRIPT
    refused((cols[0], cols[1], far))                       # a word index at n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))                       # out of (work, fan_ix) order
    refused(cols, hi=4097, code=abi.FS_E_UNSUPPORTED)
    refused(cols, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED, rows=False)
    # four tables of 4096 x 2^19 words: both factors named, and what to do
    refused(cols, lo=1, hi=4096, n_script=1 << 19, code=abi.FS_E_UNSUPPORTED, rows=False,
            says="4096 lengths (max_words - min_length + 1) x 524288 script words")
    with pytest.raises(_lib.FsError, match="lower max_words"):
        fragments.find_fragments(*cols, 3, 1 << 19, 6, 0, 2, 1, 4096)
    L = _lib.load()
    n_frags, n_active = C.c_uint64(0), C.c_uint64(0)
    none = np.zeros(1, dtype=abi.FRAGMENT_DTYPE)
    assert _call(L, cols, 3, none, 0, n_frags, none, 0, n_active,
                 n_rows=1 << 32) == abi.FS_E_UNSUPPORTED  # (refused before a record is read)
    check(index, monkeypatch, cols, 3, m=6, paths=PATHS[:1], some=False)   # (columns accepted)


# ---- the counts of the sibling commands on the same records -------------------------------

def test_works_are_whole_works_of_lines_depth_of_quotes_and_covered_of_pairs(index):
    cols, n_works = random_works(70, seed=31, hi=90, most=4)
    found, works = fragments.find_fragments(*cols, n_works, N_SCRIPT, 3, 1, 2, 1, 128)
    assert len(found) > 50
    # a line table that has the fragment as a line
    top = found[np.argsort(-found["works"].astype(np.int64), kind="stable")[:6]]
    for f in top:
        a, b = int(f["first"]), int(f["last"])
        table = sorted({0, a, b + 1, N_SCRIPT})
        got, _, _ = lines.find_lines(*cols, n_works, N_SCRIPT, table, 3, 1, 50)
        assert got["whole_works"][table.index(a)] == f["works"]
    # a one-word fragment's works are the word's depth
    comb = np.zeros(len(cols[0]))
    words, _ = quotes.find_quotes(*cols, comb, n_works, N_SCRIPT, 3, 1, 1)
    one = found[found["first"] == found["last"]]
    assert (words["n_passage_works"][one["first"]] == one["works"]).all()
    # some one-word fragment exists where the depth has a peak of one word
    depth = words["n_passage_works"].astype(np.int64)
    peaks = [o for o in range(1, N_SCRIPT - 1)
             if depth[o] >= 2 and depth[o - 1] < depth[o] > depth[o + 1]]
    assert set(peaks) <= set(one["first"].tolist())
    pair_works, _ = pairs.find_pairs(*cols, n_works, N_SCRIPT, 3, 1, 1 << 30)
    assert len(works) == 70
    assert (pair_works["covered"][works["work"]] == works["covered"]).all()
    assert pair_works["covered"].sum() == works["covered"].sum()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,m,g,k,lo,hi,top", mfg.CASES)
def test_command_on_the_golden_input(tmp_path, case, m, g, k, lo, hi, top, reader):
    src = os.path.join(GOLDEN, mfg.INPUT)
    prefix = str(tmp_path / "p")
    assert main(["fragments", src, "-o", prefix, "--min-words", str(m), "--max-gap", str(g),
                 "--min-works", str(k), "--min-length", str(lo), "--max-words", str(hi),
                 "--top", str(top), "--reader", reader]) == 0
    got = tuple(open(p, "rb").read() for p in fragments.output_names(src, prefix))
    with open(src, newline="", encoding="utf-8") as fh:
        want = fr.fragments_csv(fh.read(), m, g, k, lo, hi, top)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mfg.golden_names(case), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


@pytest.mark.parametrize("reader", ["device", "python"])
def test_command_takes_the_default_prefix_and_names_a_word_with_two_labels(tmp_path, reader):
    import shutil
    src = str(tmp_path / "m.csv")
    shutil.copy(os.path.join(GOLDEN, mfg.INPUT), src)
    assert main(["fragments", src, "--reader", reader]) == 0
    with open(src, newline="", encoding="utf-8") as fh:
        text = fh.read()
    for path, part in zip(fragments.output_names(src), fr.fragments_csv(text)):
        with open(path, "rb") as fh:
            assert fh.read() == part.encode("utf-8"), path
    with open(src, "w", newline="", encoding="utf-8") as fh:
        fh.write(text.replace(",7,bad,", ",7,good,", 1))
    with pytest.raises(SystemExit) as e:
        main(["fragments", src, "--reader", reader])
    assert str(e.value.code).startswith("ao3.py fragments: error: script word 7 has two words")
