"""`passages` on the GPU: fs_passages / fs_passages_rows against the restated contract
(tests/passages_restated.py), floats compared bit for bit; the planted copies of a synthetic
corpus found after a real search; `ao3.py passages` against the committed expected CSVs."""

import ctypes as C
import datetime
import os
from collections import Counter

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, passages, synth
from fandom_search_amd.cli import main
from tests import passages_restated as pr
from tests.golden import make_passages_golden as mpg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 4096                 # records per workgroup of the kernels
SCAN = 1024 * TILE          # records per chunk of the one-workgroup scan


def oracle(work, fan, orig, dist, comb, m, g):
    recs = list(zip(work.tolist(), fan.tolist(), orig.tolist(), dist.tolist(), comb.tolist()))
    want = pr.passages(recs, m, g)
    out = np.zeros(len(want), dtype=abi.PASSAGE_DTYPE)
    for k, p in enumerate(want):
        out[k] = tuple(p[name] for name in abi.PASSAGE_DTYPE.names)
    return out


def assert_passages_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for name in abi.PASSAGE_DTYPE.names:
        a, b = got[name], want[name]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, (name, int(bad[0]), got[bad[0]], want[bad[0]])


def random_records(n, seed, cont=0.8, nan=0.02):
    """n records sorted by (work, fan_ix): diagonal steps most of the time, with repeats, gaps,
    script jumps backwards and forwards, new works, NaN, -0.0 and 0.0."""
    rng = np.random.default_rng(seed)
    work = np.cumsum(rng.random(n) < 0.01).astype(np.int64)
    fstep = rng.choice([0, 1, 2, 3], size=n, p=[0.05, 0.8, 0.1, 0.05])
    fan = np.cumsum(fstep).astype(np.int64)
    ostep = np.where(rng.random(n) < cont, fstep, rng.integers(-50, 50, size=n))
    orig = np.cumsum(ostep) + 1000 + 50 * n
    orig = np.minimum(orig, (1 << 32) - 1)
    dist = rng.random(n) * 0.1 - 0.01
    comb = dist * rng.integers(0, 8, size=n)
    for col in (dist, comb):
        r = rng.random(n)
        col[r < nan] = np.nan
        col[(r >= nan) & (r < 2 * nan)] = -0.0
        col[(r >= 2 * nan) & (r < 3 * nan)] = 0.0
    return work.astype(np.uint32), fan.astype(np.uint32), orig.astype(np.uint32), dist, comb


def check(cols, m, g):
    got = passages.find_passages(*cols, min_words=m, max_gap=g)
    assert_passages_equal(got, oracle(*cols, m, g))
    return got


def test_zero_and_one_row():
    empty = [np.zeros(0, np.uint32)] * 3 + [np.zeros(0)] * 2
    assert len(passages.find_passages(*empty)) == 0
    one = (np.array([3], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32),
           np.array([np.nan]), np.array([-0.0]))
    got = check(one, 1, 0)
    assert len(got) == 1 and got["n_exact"][0] == 1
    assert len(check(one, 2, 0)) == 0


@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1,
                               3 * TILE + 7, 1024 * TILE // 3])
def test_sizes_around_workgroup_boundaries(n):
    rng = np.random.default_rng(n)
    for m, g in [(1, 0), (int(rng.integers(2, 9)), int(rng.integers(0, 3)))]:
        check(random_records(n, seed=n + m), m, g)


@pytest.mark.parametrize("n", [SCAN - 1, SCAN + 1])
def test_sizes_around_the_scan_chunk(n):
    check(random_records(n, seed=n, cont=0.0), 1, 0)         # mostly heads: runs cross it too


def test_random_parameters():
    rng = np.random.default_rng(2024)
    for k in range(12):
        n = int(rng.integers(1, 50_000))
        cols = random_records(n, seed=k, cont=float(rng.random()), nan=float(rng.random()) * 0.2)
        check(cols, int(rng.integers(1, 13)), int(rng.integers(0, 4)))


def test_ten_million_rows():
    check(random_records(10_000_000, seed=10), 6, 0)


def test_one_run_of_three_million_records():
    n = 3_000_000
    rng = np.random.default_rng(3)
    work = np.zeros(n, np.uint32)
    fan = np.arange(n, dtype=np.uint32)
    orig = np.arange(n, dtype=np.uint32) + 17
    dist = rng.random(n) * 1e-3
    comb = dist * 3
    dist[rng.integers(0, n, 100)] = np.nan
    comb[rng.integers(0, n, 100)] = -0.0
    got = check((work, fan, orig, dist, comb), 6, 0)
    assert len(got) == 1 and got["n_words"][0] == n
    # the same run split into a long and many short ones
    orig[n // 2:] += 5
    orig[::1000] = 0
    check((work, fan, orig, dist, comb), 1, 0)


def test_all_heads():
    n = SCAN + 3
    work = np.arange(n, dtype=np.uint32)
    cols = (work, work, work, np.ones(n), np.zeros(n))
    got = check(cols, 1, 0)
    assert len(got) == n
    assert len(passages.find_passages(*cols, min_words=2)) == 0


def test_unsorted_input_is_refused():
    work, fan, orig, dist, comb = random_records(10_000, seed=5)
    fan = fan.copy()
    fan[7000], fan[7001] = fan[7001] + 1, fan[7000]
    with pytest.raises(_lib.FsError) as e:
        passages.find_passages(work, fan, orig, dist, comb)
    assert e.value.code == abi.FS_E_INVALID
    work = work.copy()
    work[9000] = 0
    with pytest.raises(_lib.FsError) as e:
        passages.find_passages(work, np.arange(10_000, dtype=np.uint32), orig, dist, comb)
    assert e.value.code == abi.FS_E_INVALID


def test_capacity_then_success():
    cols = [abi.as_u32(c) for c in random_records(20_000, seed=8)[:3]] + \
           [np.ascontiguousarray(c) for c in random_records(20_000, seed=8)[3:]]
    want = oracle(*cols, 3, 1)
    assert len(want) > 2
    L = _lib.load()
    ptrs = [abi.ptr(c, C.c_uint32) for c in cols[:3]] + [abi.ptr(c, C.c_double) for c in cols[3:]]
    out = np.zeros(len(want), dtype=abi.PASSAGE_DTYPE)
    n = C.c_uint64(0)
    rc = L.fs_passages(0, *ptrs, len(cols[0]), 3, 1, out.ctypes.data_as(C.c_void_p),
                       len(want) - 1, C.byref(n))
    assert rc == abi.FS_E_CAPACITY and n.value == len(want)
    rc = L.fs_passages(0, *ptrs, len(cols[0]), 3, 1, out.ctypes.data_as(C.c_void_p),
                       len(want), C.byref(n))
    assert rc == abi.FS_OK and n.value == len(want)
    assert_passages_equal(out, want)


# ---- host columns and device records are one path ---------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257])            # around the pack kernel's workgroup
def test_host_columns_equal_device_records_with_another_lev(n, synth_base):
    """fs_passages packs its columns into fs_row records on the device: the passages equal, byte
    for byte, fs_passages_rows over the same records built on the host with lev = 7 (lev is not
    read; NaN, -0.0 and 0.0 arrive as they left)."""
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    script = synth.script_tokens(64)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    cols = random_records(n, seed=n, nan=0.1)
    for col in cols[3:]:                                     # NaN, -0.0 and 0.0 are among them
        zeros = col[col == 0]
        assert n == 1 or (np.isnan(col).any() and np.signbit(zeros).any()
                          and not np.signbit(zeros).all())
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    for name, col in zip(("work", "fan_ix", "orig_ix", "dist", "comb"), cols):
        rows[name] = col
    rows["lev"] = 7
    assert rows["dist"].view(np.uint64).tolist() == cols[3].view(np.uint64).tolist()
    buf = torch.from_numpy(rows.view(np.uint8)).cuda()
    torch_ready()
    for m, g in ((1, 0), (2, 1)):
        host = passages.find_passages(*cols, min_words=m, max_gap=g)
        dev = ix.passages_device(buf.data_ptr(), n, min_words=m, max_gap=g)
        assert host.tobytes() == dev.tobytes()
        assert len(host) > 0 or m > n
    ix.close()


# ---- after a real search ---------------------------------------------------------------

def planted(work_idx, n_tokens, script, vocab_size=synth.VOCAB_SIZE):
    """The spans synth.fanwork_tokens copies into a work: (src, dst, length, replaced at or
    None), drawn from the same generator in the same order."""
    rng = np.random.default_rng(1_000_003 * int(work_idx) + 17)
    synth._draw(rng, n_tokens, vocab_size)
    out = []
    for _ in range(int(rng.poisson(2.0))):
        length = int(rng.integers(6, 25))
        if length > n_tokens or length > len(script):
            continue
        src = int(rng.integers(0, len(script) - length + 1))
        dst = int(rng.integers(0, n_tokens - length + 1))
        at = None
        if rng.random() < 0.1:
            at = int(rng.integers(0, length))
            rng.integers(0, vocab_size - 1)
        out.append((src, dst, length, at))
    return out


def expected_spans(work_idx, n_tokens, script, n, repeated):
    """(G = 0 passages, G = 1 passages) the clean plants of one work must give, each a list of
    (fan start, words, script start)."""
    tok = synth.fanwork_tokens(work_idx, n_tokens, script)
    plants = planted(work_idx, n_tokens, script)
    g0, g1 = [], []
    for k, (src, dst, length, at) in enumerate(plants):
        if any(j != k and d < dst + length + 1 and dst - 1 < d + ln
               for j, (_, d, ln, _) in enumerate(plants)):
            continue                                      # overlaps or touches another plant
        if any(script[src + i:src + i + n].tobytes() in repeated for i in range(length - n + 1)):
            continue                                      # an n-gram occurs twice in the script
        if (dst > 0 and src > 0 and tok[dst - 1] == script[src - 1]) or \
           (dst + length < n_tokens and src + length < len(script)
                and tok[dst + length] == script[src + length]):
            continue                                      # the copy continues by chance
        if at is None:
            g0.append((dst, length, src))
            g1.append((dst, length, src))
        elif at >= n and length - at - 1 >= n:
            g0 += [(dst, at, src), (dst + at + 1, length - at - 1, src + at + 1)]
            g1.append((dst, length - 1, src))
    return g0, g1


def repeated_ngrams(script, n):
    c = Counter(script[i:i + n].tobytes() for i in range(len(script) - n + 1))
    return {k for k, v in c.items() if v > 1}


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
    cols = (rows["work"], rows["fan_ix"], rows["orig_ix"], rows["dist"], rows["comb"])
    repeated = repeated_ngrams(script, n)
    found = {}
    for g in (0, 1):
        dev = ix.passages_device(buf.data_ptr(), n_rows, min_words=n, max_gap=g)
        host = passages.find_passages(*cols, min_words=n, max_gap=g)
        assert_passages_equal(dev, host)
        assert_passages_equal(host, oracle(*cols, n, g))
        found[g] = {(int(rows["work"][p["first"]]), int(rows["fan_ix"][p["first"]])):
                    (int(p["n_words"]), int(rows["orig_ix"][p["first"]])) for p in host}
        # the caller's own device buffer, too small first
        k = len(host)
        out = torch.zeros(k * 48, dtype=torch.uint8, device="cuda")
        torch_ready()
        with pytest.raises(_lib.FsError) as e:
            ix.passages_device(buf.data_ptr(), n_rows, n, g, out_ptr=out.data_ptr(), cap=k - 1)
        assert e.value.required == k
        assert ix.passages_device(buf.data_ptr(), n_rows, n, g, out_ptr=out.data_ptr(), cap=k) == k
        assert_passages_equal(out.cpu().numpy().view(abi.PASSAGE_DTYPE), host)
    checked = 0
    for w in range(n_works):
        g0, g1 = expected_spans(w, per, script, n, repeated)
        for g, spans in ((0, g0), (1, g1)):
            for dst, length, src in spans:
                assert found[g].get((w, dst)) == (length, src), (w, g, dst, length, src)
                checked += 1
    assert checked > 200
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

@pytest.mark.parametrize("case,src,m,g", mpg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g):
    out = tmp_path / "p.csv"
    assert main(["passages", os.path.join(GOLDEN, src), "-o", str(out), "--min-words", str(m),
                 "--max-gap", str(g)]) == 0
    with open(os.path.join(GOLDEN, mpg.golden_name(case, m, g)), "rb") as fh:
        assert out.read_bytes() == fh.read()


def test_search_then_passages(tmp_path, monkeypatch, synth_base):
    import csv
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
    assert main(["passages", dated]) == 0
    with open(dated[:-4] + "-passages.csv", newline="", encoding="utf-8") as fh:
        table = list(csv.reader(fh))
    assert table[0] == passages.PASSAGE_FIELDS
    got = {(os.path.basename(r[0]), int(r[1])): (int(r[5]), int(r[3]), int(r[2]), r[13], r[14])
           for r in table[1:]}
    repeated = repeated_ngrams(script, 6)
    checked = 0
    for w in range(n_works):
        for dst, length, src in expected_spans(w, per, script, 6, repeated)[0]:
            text = " ".join(words[int(t)] for t in script[src:src + length])
            assert got.get((synth.work_name(w), dst)) == \
                (length, src, dst + length - 1, text, text), (w, dst)
            checked += 1
    assert checked > 20
