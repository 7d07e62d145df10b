"""`clusters` on the GPU: fs_clusters / fs_clusters_rows against the restated contract
(tests/clusters_restated.py), every field of every work and family compared for equality;
numbers of works, of column tiles and of script words around every size the kernels treat
differently; topologies whose roots are met late; the planted copies of a synthetic corpus after
a real search; `ao3.py clusters` byte for byte against the oracle's two files."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, clusters, synth
from fandom_search_amd.cli import main
from tests import clusters_restated as cr
from tests.golden import make_clusters_golden as mcg
from tests.test_gpu_pairs import CHUNK, K_SLICE, TILE, from_spans, interleaved, records
from tests.test_gpu_passages import expected_spans, repeated_ngrams

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE = abi.FS_NONE


def oracle(cols, n_works, n_script, m, g, s, j, z, p):
    recs = list(zip(*(c.tolist() for c in cols)))
    works, found = cr.clusters(recs, n_works, n_script, m, g, s, j, z, p)
    w = np.zeros(n_works, dtype=abi.CLUSTER_WORK_DTYPE)
    for name in cr.WORK_KEYS:
        w[name] = [d[name] for d in works]
    c = np.zeros(len(found), dtype=abi.CLUSTER_DTYPE)
    for name in cr.CLUSTER_KEYS:
        c[name] = [d[name] for d in found]
    return w, c


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.CLUSTER_WORK_DTYPE, abi.CLUSTER_DTYPE)):
        assert len(a) == len(b), (len(a), len(b))
        for name in dt.names:                              # (the reserved word, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def check(cols, n_works, n_script, m=6, g=0, s=6, j=50, z=2, p=50):
    got = clusters.find_clusters(*cols, n_works, n_script, m, g, s, j, z, p)
    assert_equal(got, oracle(cols, n_works, n_script, m, g, s, j, z, p))
    return got


def shuffled(spans_of, seed, first=None):
    """The same works under other numbers, so that a family's smallest work is not the one its
    links are met from first; `first`: the work that becomes work 0."""
    order = np.random.default_rng(seed).permutation(len(spans_of)).tolist()
    if first is not None:
        order.remove(first)
        order.insert(0, first)
    return [spans_of[k] for k in order]


# ---- sizes ------------------------------------------------------------------------------

def test_no_records_and_one_record():
    empty = (np.zeros(0, np.uint32),) * 3
    works, found = check(empty, 3, 10)
    assert works.tolist() == [(0, NONE, 0, NONE, 0, NONE, 0, 0)] * 3 and len(found) == 0
    works, found = check(empty, 0, 0)
    assert len(works) == 0 and len(found) == 0
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32))
    works, found = check(one, 3, 10, m=1, s=1, z=1)
    assert works[1].tolist() == (1, 1, 1, 0, 0, NONE, 0, 0)
    assert found.tolist() == [(1, 1, 0, 1, 0, 1, 1, 1, 9, 9, 1, 0)]
    works, found = check(one, 3, 10, m=1, s=1, z=2)
    assert len(found) == 0 and works[1]["cluster"] == NONE and works[1]["size"] == 1
    works, found = check(one, 3, 10, m=2, s=1, z=1)
    assert not works["covered"].any() and len(found) == 0


@pytest.mark.parametrize("n_active", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_active_works_around_the_tile(n_active):
    n_script = 300
    spans_of = interleaved(n_active, lambda k, rng: [
        (int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))
        for _ in range(int(rng.integers(1, 4)))], seed=n_active)
    cols = from_spans(spans_of)
    assert len(spans_of) > n_active + 1
    works, found = check(cols, len(spans_of), n_script, m=3, s=1, j=0, z=1)
    assert (works["covered"] > 0).sum() == n_active == found["n_works"].sum()
    check(cols, len(spans_of), n_script, m=3, s=4, j=30, z=2)


@pytest.mark.parametrize("tiles", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_column_tiles_around_a_chunk(tiles):
    n_active = (tiles - 1) * TILE + 5
    rng = np.random.default_rng(tiles)
    spans_of = [[(int(rng.integers(0, 59)), int(rng.integers(1, 3)))] for _ in range(n_active)]
    cols = from_spans(spans_of)
    works, found = check(cols, n_active, 60, m=1, s=1, j=50, z=1)
    assert found["n_works"].sum() == n_active and works["links"].sum() > 1000
    assert works["root"][n_active - 1] < (tiles - 2) * TILE   # a link across the chunks
    check(cols, n_active, 60, m=1, s=2, j=0, z=2)


@pytest.mark.parametrize("n_script", [1, 63, 64, 65, 64 * K_SLICE - 1, 64 * K_SLICE,
                                      64 * K_SLICE + 1])
def test_script_sizes_around_a_word_and_a_slice(n_script):
    sizes = np.random.default_rng(n_script).integers(0, 60, size=70)
    sizes[[3, 66]] = 5
    cols = records(sizes, n_script, seed=n_script)
    # the last script word, the last bit of the last 64-bit word, covered by two linked works
    for w in (3, 66):
        at = int(np.nonzero(cols[0] == w)[0][0])
        cols[2][at] = n_script - 1
    works, found = check(cols, 70, n_script, m=1, s=1, j=0, z=1, p=1)
    assert works["root"][3] == works["root"][66] and works["links"][66] >= 1
    if n_script > 1:
        check(cols, 70, n_script, m=3, g=1, s=2, j=20, z=2, p=50)


# ---- topologies -------------------------------------------------------------------------

def test_a_path_of_200_works():
    # work k covers 10 k .. 10 k + 11: two words with each neighbour
    path = [[(10 * k, 12)] for k in range(200)]
    spans_of = shuffled(path, seed=1, first=57)
    works, found = check(from_spans(spans_of), 200, 2100, m=3, s=2, j=0, z=2, p=50)
    assert found.tolist() == [(0, 200, 199, found[0]["hub"], 2, 2002, 0, 2, found[0]["peak_first"],
                               NONE, 0, 0)]
    assert (works["root"] == 0).all() and (works["size"] == 200).all()
    assert sorted(works["links"].tolist()) == [1, 1] + [2] * 198
    check(from_spans(spans_of), 200, 2100, m=3, s=3, j=0, z=1)    # nobody is linked


def test_a_star():
    # the centre covers 0..399; the leaves ten words each, no two of them the same
    star = [[(0, 400)]] + [[(10 * k, 10)] for k in range(40)]
    spans_of = shuffled(star, seed=2)
    centre = spans_of.index(star[0])
    assert centre != 0
    works, found = check(from_spans(spans_of), 41, 400, m=3, s=10, j=2, z=2, p=1)
    assert found.tolist() == [(0, 41, 40, centre, 40, 400, 400, 2, 0, 0, 400, 0)]
    assert works["best"][centre] == 0 and (np.delete(works["best"], centre) == centre).all()
    # at 3 per cent no leaf reaches the centre: 10 of 400
    works, found = check(from_spans(spans_of), 41, 400, m=3, s=10, j=3, z=1)
    assert len(found) == 41 and not works["links"].any()


def test_129_identical_works():
    spans_of = interleaved(129, lambda k, rng: [(70, 9), (120, 3)], seed=3)
    works, found = check(from_spans(spans_of), len(spans_of), 300, m=3, s=12, j=100, z=2, p=100)
    active = works["covered"] > 0
    assert (works["links"][active] == 128).all()
    assert len(found) == 1 and found[0]["n_links"] == 129 * 128 // 2
    assert found[0]["common"] == found[0]["covered"] == 12 and found[0]["peak"] == 129
    assert (found[0]["run_first"], found[0]["run_words"]) == (70, 9)


@pytest.mark.parametrize("short", [0, 1])
def test_two_cliques_joined_at_the_jaccard_threshold(short):
    # five works on 0..19 and five on 100..119, each clique with a bridge that covers twelve of
    # its words; the bridges cover 20 words each and share 8 or 7 around word 50: at 25 per
    # cent 8 of a union of 32 links, 7 of 33 does not
    left = [[(0, 20)] for _ in range(5)] + [[(0, 12), (50, 8 - short), (70, short)]]
    right = [[(100, 20)] for _ in range(5)] + [[(100, 12), (50, 8)]]
    spans_of = shuffled(left + right, seed=4)
    cols = from_spans(spans_of)
    works, found = check(cols, 12, 200, m=1, s=1, j=25, z=2, p=50)
    assert len(found) == 2 - (short == 0)
    assert sorted(found["n_works"].tolist()) == ([12] if short == 0 else [6, 6])
    assert found["n_links"].sum() == 2 * 15 + (short == 0)


def test_a_family_in_three_tiles():
    # 150 works with a passage of their own each, but works 5, 70 and 140 quote one line
    spans_of = [[(20 * k, 8)] for k in range(150)]
    for w in (5, 70, 140):
        spans_of[w] = [(3100, 9)]
    works, found = check(from_spans(spans_of), 150, 3200, m=3, s=6, j=50, z=2, p=100)
    assert found.tolist() == [(5, 3, 3, 5, 2, 9, 9, 3, 3100, 3100, 9, 0)]
    assert works["cluster"][[5, 70, 140]].tolist() == [0, 0, 0]
    assert (works["cluster"] == NONE).sum() == 147


def test_hundreds_of_families_of_two():
    n = 300
    twins = [[(12 * (k // 2), 7 + k % 2)] for k in range(2 * n)]
    spans_of = shuffled(twins, seed=6)
    works, found = check(from_spans(spans_of), 2 * n, 12 * n, m=3, s=6, j=50, z=2, p=100)
    assert len(found) == n and (found["n_works"] == 2).all() and (found["n_links"] == 1).all()
    assert (found["common"] == 7).all() and (found["covered"] == 8).all()
    assert (np.diff(found["root"].astype(np.int64)) > 0).all()
    assert sorted(works["cluster"].tolist()) == sorted(list(range(n)) * 2)


# ---- sweeps -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def random_input():
    sizes = np.random.default_rng(12).integers(0, 80, size=150)
    return records(sizes, 400, seed=12)


def test_min_jaccard_sweep_over_one_input(random_input):
    roots = {}
    for j in (0, 50, 100):
        works, found = check(random_input, 150, 400, m=3, s=2, j=j, z=1)
        roots[j] = works["root"]
    assert len(set(roots[0].tolist())) < len(set(roots[50].tolist())) <= len(set(roots[100].tolist()))
    # a family at a higher threshold lies inside one family at the lower one
    for lo, hi in ((0, 50), (50, 100)):
        inside = {}
        for w in range(150):
            assert inside.setdefault(int(roots[hi][w]), int(roots[lo][w])) == int(roots[lo][w])


@pytest.mark.parametrize("z", [1, 2, 5])
def test_min_size_sweep(random_input, z):
    works, found = check(random_input, 150, 400, m=3, s=4, j=10, z=z)
    assert (found["n_works"] >= z).all() and len(found) > 0
    listed = works["cluster"] != NONE
    assert ((works["size"] >= z) == listed).all()


@pytest.mark.parametrize("p", [1, 50, 100])
def test_common_pct_sweep(random_input, p):
    works, found = check(random_input, 150, 400, m=3, s=4, j=10, z=2, p=p)
    if p == 1:
        assert (found["common"] == found["covered"]).all()
    assert (found["common"] <= found["covered"]).all()


# ---- calls ------------------------------------------------------------------------------

def _call(L, cols, n_works, n_script, params, works, found, cap, n, n_rows=None):
    m, s, j, z, p = params
    return L.fs_clusters(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                         abi.ptr(cols[2], C.c_uint32), len(cols[0]) if n_rows is None else n_rows,
                         n_works, n_script, m, 0, s, j, z, p, works.ctypes.data_as(C.c_void_p),
                         found.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(n))


def test_capacity_too_small_by_one_exact_and_zero(random_input):
    cols = [np.ascontiguousarray(c) for c in random_input]
    params = (3, 2, 50, 1, 50)
    want = oracle(cols, 150, 400, 3, 0, *params[1:])
    k = len(want[1])
    assert k > 10
    L = _lib.load()
    works = np.zeros(150, dtype=abi.CLUSTER_WORK_DTYPE)
    found = np.zeros(k, dtype=abi.CLUSTER_DTYPE)
    n = C.c_uint64(0)
    for cap in (k - 1, 0):
        works[:] = 0
        assert _call(L, cols, 150, 400, params, works, found, cap, n) == abi.FS_E_CAPACITY
        assert n.value == k
        assert_equal((works, want[1]), want)               # the works are complete
        assert not found["n_works"].any()                  # the clusters untouched
    assert _call(L, cols, 150, 400, params, works, found, k, n) == abi.FS_OK and n.value == k
    assert_equal((works, found), want)


def test_refusals():
    """include/fandom_search.h.  The accepted side of FS_CLUSTERS_MAX_BYTES, tables of 1 GiB, is
    not tested: only that one row of 64-bit words more is refused.  The count moves a row
    (nk * 8 bytes) at a time, so a row is the smallest step above the limit; a single 64-bit
    word above it would take nk = 1 and about 9 * 10^7 works with a passage."""
    cols = records([300, 500, 200], 1000, seed=9)

    def refused(c, n_works=3, n_script=1000, m=6, s=6, j=50, z=2, p=50, code=abi.FS_E_INVALID):
        with pytest.raises(_lib.FsError) as e:
            clusters.find_clusters(*c, n_works, n_script, m, 0, s, j, z, p)
        assert e.value.code == code
    refused(cols, m=0)
    refused(cols, s=0)
    refused(cols, z=0)
    refused(cols, p=0)
    refused(cols, p=101)
    refused(cols, j=101)
    refused(cols, n_works=2)                               # a work >= n_works
    refused(cols, n_script=int(cols[2].max()))             # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2]))
    refused(cols, n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED)
    L = _lib.load()
    n = C.c_uint64(0)
    works = np.zeros(3, dtype=abi.CLUSTER_WORK_DTYPE)
    rc = _call(L, cols, 3, 1000, (6, 6, 50, 2, 50), works, works, 0, n, n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(cols, 3, 1000)                                   # and the same columns are accepted
    # 21 846 works of one record each, a passage at --min-words 1, over 2^18 script words, in
    # families of two or more: 21 846 coverage rows and at most 10 923 rows of masks, of 4 096
    # words of 8 bytes: one row above FS_CLUSTERS_MAX_BYTES
    nk = (1 << 18) // 64
    many = 21846
    assert (many + many // 2) * nk * 8 == abi.FS_CLUSTERS_MAX_BYTES + nk * 8
    one = (np.arange(many, dtype=np.uint32), np.zeros(many, np.uint32),
           np.arange(many, dtype=np.uint32) % 5000)
    refused(one, n_works=many, n_script=1 << 18, m=1, s=1, code=abi.FS_E_UNSUPPORTED)
    # the same columns, accepted over a smaller script: a script word is a family
    works, found = clusters.find_clusters(*one, many, 5000, 1, 0, 1, 100, 2, 100)
    assert (works["covered"] == 1).all() and len(found) == 5000
    assert (found["root"] == np.arange(5000)).all() and (found["covered"] == 1).all()
    assert sorted(set(found["n_works"].tolist())) == [4, 5]
    assert (works["root"] == np.arange(many) % 5000).all()


# ---- after a real search ---------------------------------------------------------------

def test_device_rows_after_a_search(synth_base):
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
    for g, s, j, z, p in ((0, 6, 0, 2, 50), (1, 1, 30, 1, 100)):
        dev = ix.clusters_device(buf.data_ptr(), n_rows, n_works, n, g, s, j, z, p)
        host = clusters.find_clusters(*cols, n_works, len(script), n, g, s, j, z, p)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, len(script), n, g, s, j, z, p))
        if j == 0:
            first = dev
    # the caller's own device buffers, the clusters' too small by one first
    works, found = first
    k = len(found)
    assert k >= 1
    d_works = torch.zeros(n_works * 32, dtype=torch.uint8, device="cuda")
    d_found = torch.zeros(k * 48, dtype=torch.uint8, device="cuda")
    torch_ready()
    ptrs = (d_works.data_ptr(), d_found.data_ptr())
    with pytest.raises(_lib.FsError) as e:
        ix.clusters_device(buf.data_ptr(), n_rows, n_works, n, 0, 6, 0, out_ptrs=ptrs, cap=k - 1)
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == k
    assert (d_works.cpu().numpy().view(abi.CLUSTER_WORK_DTYPE) == works).all()
    assert not d_found.cpu().numpy().any()
    assert ix.clusters_device(buf.data_ptr(), n_rows, n_works, n, 0, 6, 0, out_ptrs=ptrs,
                              cap=k) == k
    assert (d_found.cpu().numpy().view(abi.CLUSTER_DTYPE) == found).all()
    ms = (C.c_double * 5)()
    assert _lib.load().fs_clusters_times(ms) == abi.FS_OK and all(t > 0 for t in ms)
    # no records: works without coverage on the device
    assert ix.clusters_device(buf.data_ptr(), 0, n_works, n, out_ptrs=ptrs, cap=k) == 0
    none = d_works.cpu().numpy().view(abi.CLUSTER_WORK_DTYPE)
    assert (none["root"] == NONE).all() and not none["covered"].any()
    # two works planted with verbatim spans of the script that have n words or more in common
    # are linked, so in one family, at min_jaccard 0 (the corpus plants no span twice whole)
    repeated = repeated_ngrams(script, n)
    planted = []
    for w in range(n_works):
        planted += [(src, src + length, w) for _, length, src in
                    expected_spans(w, per, script, n, repeated)[0] if length >= n]
    checked = 0
    for i, (s0, e0, w0) in enumerate(planted):
        for s1, e1, w1 in planted[i + 1:]:
            lo, hi = max(s0, s1), min(e0, e1)
            if w0 == w1 or hi - lo < n:
                continue
            assert works["root"][w0] == works["root"][w1] != NONE
            for w in (w0, w1):
                assert works["links"][w] >= 1 and works["best_shared"][w] >= hi - lo
            checked += 1
    assert checked > 20
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

def _run_command(tmp_path, src_path, m, g, s, j, z, p, reader):
    prefix = str(tmp_path / "p")
    assert main(["clusters", src_path, "-o", prefix, "--min-words", str(m), "--max-gap", str(g),
                 "--min-shared", str(s), "--min-jaccard", str(j), "--min-size", str(z),
                 "--common", str(p), "--reader", reader]) == 0
    return tuple(open(f, "rb").read() for f in clusters.output_names(src_path, prefix))


@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,src,m,g,s,j,z,p", mcg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g, s, j, z, p, reader):
    got = _run_command(tmp_path, os.path.join(GOLDEN, src), m, g, s, j, z, p, reader)
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        want = cr.clusters_csv(fh.read(), m, g, s, j, z, p)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mcg.golden_names(case, m, g, s, j, z, p), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_search_then_clusters(tmp_path, monkeypatch, synth_base):
    from fandom_search_amd import search
    vocab = synth_base["words"]
    n_works, per = 40, 1500
    script = synth.script_tokens(3000)
    fandir = tmp_path / "fanworks"
    synth.write_corpus(str(fandir), n_works, per, script, vocab)
    (tmp_path / "script.txt").write_text(synth.script_markup(script, vocab))
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    monkeypatch.delenv("FANDOM_SEARCH_VECTORS", raising=False)
    assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--synthetic-vocab"]) == 0
    dated = "match-6gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    assert main(["clusters", dated, "--min-shared", "1", "--min-jaccard", "0",
                 "--min-size", "1"]) == 0                  # default prefix: beside the input
    with open(dated, newline="", encoding="utf-8") as fh:
        want = cr.clusters_csv(fh.read(), min_shared=1, min_jaccard=0, min_size=1)
    for path, text in zip(clusters.output_names(dated), want):
        with open(path, "rb") as fh:
            assert fh.read() == text.encode("utf-8"), path
    assert want[1].count("\r\n") > 10 and want[0].count("\r\n") > 1
