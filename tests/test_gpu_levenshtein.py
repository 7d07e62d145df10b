"""Every device implementation of Levenshtein.distance(match_str, fan_context) against a plain
DP, at the operand lengths where Myers' recurrence, the string records and the hand-over to the
scratch DP can go wrong.  The operand pairs travel through the public search (tests/levpairs.py):
the records' `lev` must equal levpairs.distance, the whole rows the C oracle's.  Integer equality
throughout, no tolerances.

Paths (switches are read when the index is created):

  exact_own         string ids of their own             lev_lane in k_scan_rows (n = 2 .. 8), else k_strbest
  exact_own_chain   FS_STR_FUSED=0                      lev_lane in k_strbest
  exact_own_wave    FS_STR_FAST=0                       lev_wave in k_matchlev
  exact_vec         string id == vector id, no tok_str  lev_wave in k_levtab / k_ctab
  exact_vecx        tok_str == tok passed               k_levtab, table hits
  exact_vecx_each   the same, FS_STR_LEVTAB=0           every distance per match
  lsh_own           FS_MODE_GENERAL, own string ids     k_lsh_lev on an index's first search, lev_wave in
                                                        k_lsh_verify on its second (_run_lsh checks both)
  lsh_own_lane      FS_LSH_LEV_LANE=2                   lev_lane_ids in k_lsh_lev
  lsh_own_wave      FS_LSH_LEV_LANE=0                   lev_wave in k_lsh_verify
  lsh_vec           FS_MODE_GENERAL, id == vector id    k_selflev, k_lsh_gramtab

The exact paths are told apart by the kernel name the library reports, the LSH paths by the
profile marks of the search itself (k_lsh_lev or not).  Nothing the library exposes tells
k_strbest from k_matchlev, or a table hit of exact_vecx from a per-hit distance: there the
switch is what the test can vouch for.
"""

import contextlib

import pytest

from fandom_search_amd import abi, synth
from tests import levpairs as lp
from tests import util

pytestmark = pytest.mark.gpu

EXACT, LSH = abi.FS_MODE_EXACT, abi.FS_MODE_GENERAL

# name: (string layout, mode, switches)
PATHS = {
    "exact_own": ("own", EXACT, {}),
    "exact_own_chain": ("own", EXACT, {"FS_STR_FUSED": "0"}),
    "exact_own_wave": ("own", EXACT, {"FS_STR_FAST": "0"}),
    "exact_vec": ("vec", EXACT, {}),
    "exact_vecx": ("vec_explicit", EXACT, {}),
    "exact_vecx_each": ("vec_explicit", EXACT, {"FS_STR_LEVTAB": "0"}),
    "lsh_own": ("own", LSH, {}),
    "lsh_own_lane": ("own", LSH, {"FS_LSH_LEV_LANE": "2"}),
    "lsh_own_wave": ("own", LSH, {"FS_LSH_LEV_LANE": "0"}),
    "lsh_vec": ("vec", LSH, {}),
}
# the fan side has no 512 limit here: one lane walks the fan text class by class
LANE_PATHS = ("exact_own", "exact_own_chain", "lsh_own_lane")


def _expected(name, layout):
    """(Built, oracle rows): tok_str == tok is the input of "vec" spelled out, so the oracle's
    rows of "vec" serve both."""
    b, want = lp.oracle_rows(name, "vec" if layout == "vec_explicit" else layout)
    if layout == "vec_explicit":
        b = b._replace(tok_str=b.tok.copy())
    return b, want


@contextlib.contextmanager
def _opened(b, path, monkeypatch):
    """(index, corpus) of `b` down `path`; the switches are set before the index is created."""
    from fandom_search_amd.engine import ScriptIndex
    layout, mode, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = abi.make_config(window_size=b.n, mode=mode)
    ix = ScriptIndex(b.script, b.swords, synth.embedding(), synth.lsh_normals(b.n), cfg=cfg)
    try:
        if mode == EXACT:
            assert ix.info["proof_ok"] == 1 and ix.info["path"] == EXACT
        yield ix, ix.corpus(b.tok, b.off, b.chars, b.coff, tok_str=b.tok_str)
    finally:
        ix.close()


def _search(ix, corpus, path):
    got, st = ix.search(corpus)
    assert st.path == PATHS[path][1], (st.path, path)
    return got.copy()


def _profiled_search(ix, corpus, n_rows):
    """One search with the library's profile marks: (rows, names of the kernels it launched).
    The rows go to a zero-filled device buffer with room for eight more than expected: a record
    has lev >= 2 (the brackets), so the zero records behind the last one prove the count."""
    import torch
    cap = n_rows + 8
    buf = torch.zeros(cap * abi.ROW_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()          # the fill is torch's, the search writes on the library's streams
    marks = [name for name, ms in ix.profile(corpus, buf.data_ptr(), cap)]
    rows = buf.cpu().numpy().view(abi.ROW_DTYPE)
    assert not rows[n_rows:].tobytes().strip(b"\0"), "more records than predicted"
    return rows[:n_rows].copy(), marks


def _check_kernel(path, b, kernel):
    """A path must not silently become another: what the library says it launches (exact
    pipeline; the LSH paths are told apart by their profile marks, _run_lsh)."""
    layout, mode, env = PATHS[path]
    classes = lp.alphabet_size(b.pairs) <= 125           # the class path exists
    fused = 2 <= b.n <= 8 and not env.get("FS_STR_FUSED") and not env.get("FS_STR_FAST")
    if layout != "vec" and not classes:
        fused = False
    if fused:
        assert kernel.startswith("k_scan_rows<%d," % b.n), kernel
    else:
        assert kernel in ("k_scan8<%d>" % b.n, "k_scan<%d>" % b.n), kernel


def _run_lsh(name, path, monkeypatch):
    """Two searches on one index, each with its profile marks.  k_lsh_lev (a lane per kept match,
    lev_lane_ids) runs where the character classes exist and FS_LSH_LEV_LANE is 2, or is unset
    and the index's last search left many windows pending -- "none yet" counts as many, so the
    first search of a default index takes it and the second, after these few hundred windows,
    computes the distances with lev_wave inside k_lsh_verify, as FS_LSH_LEV_LANE=0 always does."""
    layout, mode, env = PATHS[path]
    b, want = _expected(name, layout)
    classes = lp.alphabet_size(b.pairs) <= 125
    lane = {"2": (classes, classes), "0": (False, False)}.get(env.get("FS_LSH_LEV_LANE"), (classes, False))
    with _opened(b, path, monkeypatch) as (ix, corpus):
        kernel = ix.kernel_name(corpus)
        assert not kernel.startswith("k_scan_rows") and kernel not in ("k_scan8<%d>" % b.n, "k_scan<%d>" % b.n), kernel
        for nth in (0, 1):
            got, marks = _profiled_search(ix, corpus, len(want))
            print("%s %s search %d: %s" % (name, path, nth + 1, " ".join(marks)))
            lp.assert_predicted(got, b)
            util.assert_rows_equal(got, want)
            assert ("k_lsh_lev" in marks) == lane[nth], (nth, marks)
            assert "k_lsh_verify" in marks or "k_lsh_batch" in marks, marks


def _run(name, path, monkeypatch):
    if PATHS[path][1] == LSH:
        return _run_lsh(name, path, monkeypatch)
    b, want = _expected(name, PATHS[path][0])
    with _opened(b, path, monkeypatch) as (ix, corpus):
        kernel = ix.kernel_name(corpus)
        got = _search(ix, corpus, path)
    print("%s %s: kernel %s, %d pairs, %d rows, lev %d..%d" % (
        name, path, kernel, len(b.pairs), len(got), int(got["lev"].min()) if len(got) else 0,
        int(got["lev"].max()) if len(got) else 0))
    lp.assert_predicted(got, b)                 # lev against the plain DP, pair named on failure
    util.assert_rows_equal(got, want)           # whole rows against the C oracle
    _check_kernel(path, b, kernel)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", lp.GRID_LISTS)
def test_length_grid(name, path, monkeypatch):
    """la x lb of the issue's grid at n = 6: the whole product (13 x 17) with disjoint, two-letter
    random and shifted-copy contents, every content on the sub-grid at or below 129.  Patterns of
    32, 33 and 64 bits, texts ending on and one past a 64-column block, la == lb, one operand over
    64, both over 64 (scratch DP), 512 on either side."""
    _run(name, path, monkeypatch)


# The exact pipeline needs the n-gram proof (cos bound < 1 - threshold), which the synthetic
# vector table gives up to n = 8 only: fs_index_create refuses FS_MODE_EXACT at 9, 12 and 16.
WINDOW_RUNS = [(name, path) for name in lp.WINDOW_LISTS for path in sorted(PATHS)
               if PATHS[path][1] == LSH or lp.cases(name)[0] <= 8]


@pytest.mark.parametrize("name,path", WINDOW_RUNS)
def test_window_sizes(name, path, monkeypatch):
    """The sub-grid at window sizes 1, 2, 4, 9, 12 and 16 (n = 1 with an empty script word gives
    la = 0; at n = 16 every written-out word of lev_lane_ids runs).  Pipelines: exact indexes
    take k_scan_rows at n = 2 and 4 and the chained kernels (k_scan8 / k_scan, then k_strbest or
    k_matchlev) at n = 1; at n = 9, 12 and 16 the synthetic table has no exact proof and the LSH
    pipeline is the only one, which FS_MODE_GENERAL indexes take at every n."""
    _run(name, path, monkeypatch)


@pytest.mark.parametrize("path", sorted(PATHS))
def test_fan_word_lengths(path, monkeypatch):
    """Fan words of 0, 1, 14, 15, 16, 17, 254, 255, 256, 257 and 300 code points in the first, a
    middle and the last slot (k_strrec keeps a length byte capped at 255 and the classes of the
    first 15 code points; longer words are read from memory); at 15 and 16 the 15th and 16th
    characters decide the distance."""
    _run("words6", path, monkeypatch)


@pytest.mark.parametrize("path", LANE_PATHS)
def test_fan_text_past_512_on_lane_paths(path, monkeypatch):
    """Fan texts of 530 .. 620 code points against script windows within 64: the lane paths walk
    them whole."""
    _run("words6_long", path, monkeypatch)


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", lp.ALPHA_LISTS)
def test_alphabet_size(name, path, monkeypatch):
    """Script text of 124, 125 and 126 distinct code points, the space included: 125 is the most
    the 7 bit planes hold; at 126 the class path is off and the wave kernels take over (k_scan_rows
    gives way to the chained kernels for batches with string ids).  Same records."""
    _run(name, path, monkeypatch)


ROWS, REFUSED = "rows", "refused"

# What each path does at the limits, from reading the code.  lev_lane / lev_lane_ids walk a fan
# text of any length and refuse a distance above 1023 (the 8-byte wire records hold ten bits);
# lev_wave and lev_device hold both operands in FS_LEV_MAX = 512 code points and refuse more; a
# script window of more than 64 code points goes to lev_device on every path.  A fresh
# FS_MODE_GENERAL index takes "no search yet" for many pending windows and computes the kept
# matches in k_lsh_lev like FS_LSH_LEV_LANE=2, with or without string ids of the batch's own.
# exact_vecx* fall back from the table to lev_lane.  exact_vec leaves the table entries of
# over-long n-grams unknown and refuses a hit on one (k_gbest_known).
LIMITS = {
    "limit_d1023": {"exact_own": ROWS, "exact_own_chain": ROWS, "exact_own_wave": REFUSED,
                    "lsh_own": ROWS, "lsh_own_lane": ROWS, "lsh_own_wave": REFUSED},
    "limit_d1024": {"exact_own": REFUSED, "exact_own_chain": REFUSED, "exact_own_wave": REFUSED,
                    "lsh_own": REFUSED, "lsh_own_lane": REFUSED, "lsh_own_wave": REFUSED},
    "limit_la513_unquoted": {p: ROWS for p in PATHS},
    "limit_la513_quoted": {p: REFUSED for p in PATHS},
    "limit_lb513": {"exact_own": ROWS, "exact_own_chain": ROWS, "exact_own_wave": REFUSED,
                    "exact_vec": REFUSED, "exact_vecx": ROWS, "exact_vecx_each": ROWS,
                    "lsh_own": ROWS, "lsh_own_lane": ROWS, "lsh_own_wave": REFUSED,
                    "lsh_vec": ROWS},
}


@pytest.mark.parametrize("name,path", [(n, p) for n in lp.LIMIT_LISTS for p in sorted(LIMITS[n])])
def test_limits_never_a_wrong_number(name, path, monkeypatch):
    """A distance of exactly 1023 and 1024 behind a script window within 64; a script window of
    513 code points, unquoted and quoted; a fan text of 513: a path returns the oracle's rows or
    its search -- not the creation of the index or of the corpus -- raises FS_E_UNSUPPORTED, as
    LIMITS says, and an unquoted over-long window fails no search."""
    from fandom_search_amd import _lib
    b, want = _expected(name, PATHS[path][0])
    # (the corpus is made outside the refusal: its creation never refuses an over-long text)
    with _opened(b, path, monkeypatch) as (ix, corpus):
        if LIMITS[name][path] == ROWS:
            got = _search(ix, corpus, path)
            lp.assert_predicted(got, b)
            util.assert_rows_equal(got, want)
        else:
            with pytest.raises(_lib.FsError) as e:
                got = _search(ix, corpus, path)
                print("no error; lev", got["lev"].tolist(), "oracle", want["lev"].tolist())
            assert e.value.code == abi.FS_E_UNSUPPORTED and "512" in str(e.value)
