"""`fanon` on the GPU: fs_fanon and fs_fanon_dev against the restated contract
(tests/fanon_restated.py), every field of the four records compared for equality: K at its
bounds, works around K tokens, work boundaries, a planted phrase at every offset around the
tile edges, repetition, the bounds of --min-works and --max-share, canon, the token unions, the
hash cut down to 4 and to 0 bits, random corpora over a handful of ids, the errors, and
`ao3.py fanon` against the host restatement."""

import ctypes as C
import os
import random

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, engine
from fandom_search_amd.cli import main
from tests import fanon_restated as fr
from tests.golden import make_fanon_golden as mfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ID = abi.FS_FANON_NO_ID
DTYPES = (abi.FANON_WORK_DTYPE, abi.FANON_GRAM_DTYPE, abi.FANON_PASSAGE_DTYPE,
          abi.FANON_PHRASE_DTYPE)
KEYS = (fr.WORK_KEYS, fr.GRAM_KEYS, fr.PASSAGE_KEYS, fr.PHRASE_KEYS)


def arrays(works, scripts):
    tok = np.asarray([t for w in works for t in w], dtype=np.uint32)
    off = np.zeros(len(works) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(w) for w in works])
    canon = np.asarray([t for s in scripts for t in s], dtype=np.uint32)
    coff = np.zeros(len(scripts) + 1, dtype=np.uint64)
    coff[1:] = np.cumsum([len(s) for s in scripts])
    return tok, off, canon, coff


def n_ids_of(works, scripts=()):
    """One past the largest id of either side (a script may hold ids no work does)."""
    ids = [t for w in works for t in w] + [t for s in scripts for t in s if t != NO_ID]
    return max(ids, default=0) + 1


def oracle(works, scripts, k, min_works, max_share):
    parts = fr.fanon(works, scripts, k, min_works, max_share)
    out = []
    for part, keys, dt in zip(parts[:4], KEYS, DTYPES):
        a = np.zeros(len(part), dtype=dt)
        for name in keys:
            a[name] = [d[name] for d in part]
        out.append(a)
    return tuple(out), parts[4]


def assert_equal(got, want):
    for a, b, dt in zip(got, want, DTYPES):
        assert len(a) == len(b), (dt.names, len(a), len(b))
        for name in dt.names:
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def host_call(works, scripts, k, min_works, max_share):
    tok, off, canon, coff = arrays(works, scripts)
    got = engine.fanon(tok, off, n_ids_of(works, scripts), canon, coff, k, min_works, max_share)
    return got[:4], got[4]


def device_call(works, scripts, k, min_works, max_share):
    import torch
    tok, off, canon, coff = arrays(works, scripts)

    def dev(a):
        return torch.from_numpy(a.view(np.uint8) if len(a) else np.zeros(8, np.uint8)).to("cuda")
    d_tok, d_off, d_canon, d_coff = dev(tok), dev(off), dev(canon), dev(coff)
    engine.torch_ready()
    totals = {}
    got = engine.fanon_device(d_tok.data_ptr(), len(tok), d_off.data_ptr(), len(works),
                              n_ids_of(works, scripts), d_canon.data_ptr(), len(canon),
                              d_coff.data_ptr(), len(scripts), k, min_works, max_share,
                              totals=totals)
    return got, totals


def check(works, scripts=(), k=8, min_works=2, max_share=100):
    """Both entry points against the oracle; the oracle's records and the host's."""
    scripts = list(scripts)
    want, totals = oracle(works, scripts, k, min_works, max_share)
    got, t = host_call(works, scripts, k, min_works, max_share)
    assert_equal(got, want)
    assert t == totals
    got_d, t_d = device_call(works, scripts, k, min_works, max_share)
    assert_equal(got_d, want)
    assert t_d == totals
    return want, got


def filler(n, base):
    """n ids no other token has."""
    return list(range(base, base + n))


# ---- K bounds -------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 8, 32])
def test_k_bounds_and_works_around_k_tokens(k):
    phrase = filler(k + 3, 0)
    works = [[], phrase[:k - 1], phrase[:k], phrase[:k + 1], [], phrase, filler(5, 100) + phrase]
    want, _ = check(works, k=k)
    w, g, p, f = want
    assert w['n_positions'].tolist() == [0, 0, 1, 2, 0, 4, 9]
    assert len(g) == 4 and g['works'].tolist() == [4, 3, 2, 2]
    assert p['n_tokens'].tolist() == [k, k + 1, k + 3, k + 3] and len(f) == 3


@pytest.mark.parametrize("k", [2, 8, 32])
def test_one_work_only_and_all_works_empty(k):
    want, _ = check([filler(k, 0) * 3], k=k, min_works=1)
    assert len(want[1]) == k and want[0]['n_passages'][0] == 1
    want, _ = check([filler(k, 0) * 3], k=k)
    assert len(want[1]) == 0 and len(want[2]) == 0
    want, got = check([[], [], []], k=k)
    assert want[0]['n_tokens'].tolist() == [0, 0, 0]
    want, _ = check([filler(k - 1, 0), [], filler(k - 1, 0)], k=k)      # no position at all
    assert want[0]['n_tokens'].tolist() == [k - 1, 0, k - 1] and not want[0]['n_positions'].any()
    check([], k=k)


# ---- work boundaries ------------------------------------------------------------------------

def test_a_phrase_across_two_works_gives_no_gram():
    phrase = filler(12, 0)
    works = [filler(30, 100) + phrase[:6], phrase[6:] + filler(30, 200),
             filler(10, 300) + phrase + filler(10, 400)]
    want, _ = check(works, k=8)
    assert len(want[1]) == 0 and len(want[2]) == 0
    want, _ = check(works, k=6)          # each half is one gram of six, shared with work 2
    assert want[1]['works'].tolist() == [2, 2]
    assert [(int(p['work']), int(p['start'])) for p in want[2]] == [(0, 30), (1, 0), (2, 10), (2, 16)]


# ---- tile edges -----------------------------------------------------------------------------

@pytest.mark.parametrize("anchor", sorted({64, 256, 1024, 4096, abi.FS_FANON_TILE}))
def test_planted_phrase_around_a_tile_edge(anchor):
    phrase = filler(12, 0)
    for delta in range(-12, 2):
        start = anchor + delta
        works = [filler(start, 100) + phrase + filler(20, 10000), filler(7, 20000) + phrase]
        want, _ = check(works, k=8)
        assert len(want[1]) == 5 and len(want[3]) == 1
        assert [(int(p['work']), int(p['start']), int(p['n_tokens'])) for p in want[2]] == \
            [(0, start, 12), (1, 7, 12)]


# ---- repetition -----------------------------------------------------------------------------

def test_a_gram_ten_times_in_one_work_is_not_shared():
    gram = filler(8, 0)
    sep = iter(range(100, 200))
    work = []
    for _ in range(10):
        work += gram + [next(sep)]
    want, got = check([work, filler(40, 1000)], k=8)
    assert len(want[1]) == 0 and want[0]['shared_positions'].tolist() == [0, 0]
    want, _ = check([work, filler(40, 1000)], k=8, min_works=1)
    first = want[1][0]
    assert (int(first['works']), int(first['occurrences'])) == (1, 10)


def test_works_of_equal_tokens():
    want, _ = check([[3] * 300, [3] * 40], k=8)
    assert len(want[1]) == 1
    assert (int(want[1][0]['works']), int(want[1][0]['occurrences'])) == (2, 293 + 33)
    assert want[2]['n_tokens'].tolist() == [300, 40] and len(want[3]) == 2
    check([[3] * 300, [3] * 40, [3] * 300], k=32)


# ---- bounds ---------------------------------------------------------------------------------

def test_min_works_at_the_bound_and_one_below():
    a, b = filler(8, 0), filler(8, 50)
    works = [a + [100], a + [101], a + [102] + b, b + [103]]      # a in 3 works, b in 2
    want, _ = check(works, k=8, min_works=3)
    assert len(want[1]) == 1 and int(want[1][0]['works']) == 3
    want, _ = check(works, k=8, min_works=2)
    assert want[1]['works'].tolist() == [3, 2]
    want, _ = check(works, k=8, min_works=4)
    assert len(want[1]) == 0


def test_max_share_at_the_bound_and_one_above():
    a, b = filler(8, 0), filler(8, 50)
    # of 4 works a stands in 2 (50 %: works * 100 == 50 * n_works, not common) and b in 3
    works = [a + [100] + b, a + [101] + b, b + [102], [103] * 3]
    want, _ = check(works, k=8, max_share=50)
    assert want[1]['works'].tolist() == [2]
    assert want[0]['common_positions'].tolist() == [1, 1, 1, 0]
    want, _ = check(works, k=8, max_share=49)
    assert len(want[1]) == 0 and want[0]['common_positions'].tolist() == [2, 2, 1, 0]
    want, _ = check(works, k=8, max_share=75)
    assert want[1]['works'].tolist() == [2, 3]
    check(works, k=8, max_share=74)
    check(works, k=8, max_share=1)


# ---- canon ----------------------------------------------------------------------------------

def test_canon():
    line = filler(12, 0)
    works = [filler(5, 100) + line + filler(5, 200), filler(3, 300) + line, filler(9, 400)]
    want, _ = check(works, [filler(4, 900) + line + filler(4, 950)], k=8)
    assert len(want[1]) == 0 and want[0]['canon_positions'].tolist() == [5, 5, 0]
    assert want[0]['canon_tokens'].tolist() == [12, 12, 0]
    # the same stretch cut across two scripts: no script holds a gram of it
    want, _ = check(works, [filler(4, 900) + line[:6], line[6:] + filler(4, 950)], k=8)
    assert len(want[1]) == 5 and not want[0]['canon_positions'].any()
    # a script shorter than K, and an empty one
    want, _ = check(works, [line[:7], [], line[5:]], k=8)
    assert len(want[1]) == 5
    # a script word that is no fan token, in the middle of the line and behind it
    want, _ = check(works, [line[:5] + [NO_ID] + line[6:], line + [NO_ID]], k=8)
    assert want[0]['canon_positions'].tolist() == [5, 5, 0]
    want, _ = check(works, [line[:5] + [NO_ID] + line[6:]], k=8)
    assert not want[0]['canon_positions'].any()
    # canon and common at once
    want, _ = check(works, [line], k=8, max_share=50)
    assert want[0]['canon_positions'].tolist() == want[0]['common_positions'].tolist()


# ---- token unions ---------------------------------------------------------------------------

def test_token_unions_count_a_token_once():
    k = 4
    a, b, c = filler(4, 0), filler(4, 10), filler(6, 20)
    # work 0: positions 0 shared (a), 1 not, 2..4 shared (c's three grams start at 2): two
    # passages whose tokens overlap
    w0 = [a[0], a[1], c[0], c[1], c[2], c[3], c[4], c[5]]
    works = [w0, [a[0], a[1], c[0], c[1]] + [99], filler(3, 200) + c, b]
    want, _ = check(works, k=k)
    w = want[0][0]
    assert [(int(p['start']), int(p['n_tokens'])) for p in want[2] if p['work'] == 0] == \
        [(0, 4), (2, 6)]
    assert (int(w['shared_positions']), int(w['shared_tokens']), int(w['n_passages'])) == (4, 8, 2)
    assert (int(w['longest_start']), int(w['longest_tokens'])) == (2, 6)


# ---- random cases, and the hash ---------------------------------------------------------------

def random_case(seed):
    rng = random.Random(seed)
    n_ids = rng.randint(4, 6)
    works = [[rng.randrange(n_ids) for _ in range(rng.choice((0, 1, rng.randint(0, 200), rng.randint(0, 200))))]
             for _ in range(rng.randint(1, 50))]
    scripts = [[rng.choice((rng.randrange(n_ids), rng.randrange(n_ids), NO_ID))
                for _ in range(rng.randint(0, 12))] for _ in range(rng.randint(0, 3))]
    return (works, scripts, rng.randint(2, 5), rng.randint(1, 4),
            rng.choice((100, 100, 60, 30, 10)))


@pytest.mark.parametrize("group", range(6))
def test_random_cases(group):
    for seed in range(group * 6, group * 6 + 6):
        check(*random_case(seed))


def hash_cases():
    phrase = filler(12, 0)
    yield [filler(250, 100) + phrase + filler(20, 10000), filler(7, 20000) + phrase], [], 8, 2, 100
    yield [[3] * 300, [3] * 40], [], 8, 2, 100
    line = filler(12, 0)
    yield ([filler(5, 100) + line + filler(5, 200), filler(3, 300) + line, filler(9, 400)],
           [line[:5] + [NO_ID] + line[6:], line + [NO_ID]], 8, 2, 100)
    for seed in (8, 16, 31, 33):
        yield random_case(seed)


@pytest.mark.parametrize("bits", ["4", "0"])
def test_hash_independence(monkeypatch, bits):
    for case in hash_cases():
        monkeypatch.delenv("FS_FANON_HASH_BITS", raising=False)
        plain, _ = host_call(*case)
        want, _ = oracle(*case)
        assert_equal(plain, want)
        monkeypatch.setenv("FS_FANON_HASH_BITS", bits)
        cut, _ = host_call(*case)
        cut_d, _ = device_call(*case)
        for a, b, c in zip(plain, cut, cut_d):
            assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- errors ---------------------------------------------------------------------------------

def raw(tok, off, n_ids, canon, coff, k, min_works, max_share, caps):
    """fs_fanon with buffers of `caps` records: (code, counts, works)."""
    L = _lib.load()
    n_works = len(off) - 1
    works = np.zeros(max(1, n_works), dtype=abi.FANON_WORK_DTYPE)
    outs = [np.zeros(max(1, c), dtype=d) for c, d in zip(caps, DTYPES[1:])]
    counts = [C.c_uint64(0) for _ in range(3)]
    tok, off = abi.as_u32(tok), abi.as_u64(off)
    canon, coff = abi.as_u32(canon), abi.as_u64(coff)
    rc = L.fs_fanon(0, abi.ptr(tok if len(tok) else np.zeros(1, np.uint32), C.c_uint32),
                    abi.ptr(off, C.c_uint64), n_works, n_ids,
                    abi.ptr(canon if len(canon) else np.zeros(1, np.uint32), C.c_uint32),
                    abi.ptr(coff, C.c_uint64), len(coff) - 1, k, min_works, max_share,
                    works.ctypes.data_as(C.c_void_p),
                    outs[0].ctypes.data_as(C.c_void_p), caps[0],
                    outs[1].ctypes.data_as(C.c_void_p), caps[1],
                    outs[2].ctypes.data_as(C.c_void_p), caps[2],
                    C.byref(counts[0]), C.byref(counts[1]), C.byref(counts[2]), None, None)
    return rc, [int(c.value) for c in counts], works[:n_works]


def test_capacity_for_each_cap():
    works, scripts, k, mw, ms = random_case(8)
    want, _ = oracle(works, scripts, k, mw, ms)
    full = [len(want[1]), len(want[2]), len(want[3])]
    assert all(n > 1 for n in full)
    tok, off, canon, coff = arrays(works, scripts)
    for short in range(3):
        caps = list(full)
        caps[short] -= 1
        rc, counts, w = raw(tok, off, n_ids_of(works, scripts), canon, coff, k, mw, ms, caps)
        assert rc == abi.FS_E_CAPACITY and counts == full
        assert w.tobytes() == want[0].tobytes()
    rc, counts, _ = raw(tok, off, n_ids_of(works, scripts), canon, coff, k, mw, ms, full)
    assert rc == abi.FS_OK and counts == full


def test_max_bytes_refusal(monkeypatch):
    works, scripts, k, mw, ms = random_case(8)
    monkeypatch.setenv("FS_FANON_MAX_BYTES", "4096")
    with pytest.raises(_lib.FsError) as e:
        host_call(works, scripts, k, mw, ms)
    assert e.value.code == abi.FS_E_UNSUPPORTED
    assert "lower -n" in str(e.value) and "bytes" in str(e.value)
    with pytest.raises(_lib.FsError) as e:
        device_call(works, scripts, k, mw, ms)
    assert e.value.code == abi.FS_E_UNSUPPORTED
    monkeypatch.delenv("FS_FANON_MAX_BYTES")
    check(works, scripts, k, mw, ms)


def test_invalid_arguments():
    works = [filler(10, 0), filler(10, 0)]
    tok, off, canon, coff = arrays(works, [filler(9, 0)])
    caps = [64, 64, 64]
    ok = dict(tok=tok, off=off, n_ids=10, canon=canon, coff=coff, k=8, min_works=2, max_share=100,
              caps=caps)
    assert raw(**ok)[0] == abi.FS_OK
    for change in (dict(k=1), dict(k=33), dict(k=0), dict(min_works=0), dict(max_share=0),
                   dict(max_share=101), dict(n_ids=9),
                   dict(canon=np.asarray([0, 1, 2, 3, 4, 5, 6, 7, 10], np.uint32)),
                   dict(off=np.asarray([0, 12, 10], np.uint64)),
                   dict(off=np.asarray([1, 10, 20], np.uint64)),
                   dict(coff=np.asarray([2, 9], np.uint64))):
        assert raw(**dict(ok, **change))[0] == abi.FS_E_INVALID, change
    with pytest.raises(_lib.FsError) as e:
        device_call(works, [], 33, 2, 100)
    assert e.value.code == abi.FS_E_INVALID
    # a script word that is FS_FANON_NO_ID is none of these
    assert raw(**dict(ok, canon=np.asarray([0, 1, 2, 3, NO_ID, 5, 6, 7, 8], np.uint32)))[0] == abi.FS_OK


# ---- end to end -----------------------------------------------------------------------------

TEXTS = {
    "a.txt": "Disclaimer: I own nothing here.\n\nShe said the stars were never ours to keep, and "
             "he laughed anyway.\n",
    "b.txt": "disclaimer: i own nothing here.\nThe stars were never ours to keep, Luke.\n",
    "c.txt": "May the Force be with you, always. The stars were never ours to keep!\n",
    "d.txt": "Nothing to see.\n",
    "e.txt": "",
    "f.txt": "Disclaimer: I own nothing here.\nMay the Force be with you, always.\n",
    "g.txt": "She said the stars were never ours to keep, and he laughed anyway.\n",
    "h.txt": "One two three four five six seven eight nine ten.\n",
    "i.txt": "one two three four five six seven eight nine ten eleven\n",
    "j.txt": "Ten nine eight seven six five four three two one.\n",
    "k.txt": "he laughed anyway. He laughed anyway. He laughed anyway.\n",
    "l.txt": "Disclaimer: I own nothing here.\n",
}
SCRIPT = ("SCENE_NUMBER<<1>>\nCHARACTER_NAME<<OBI-WAN>>\n"
          "LINE<<May the Force be with you, always.>>\n")


@pytest.mark.parametrize("options", [[], ["--length", "4", "--min-works", "3", "--keep-case"],
                                     ["--length", "3", "--max-share", "30", "--top", "2"]])
def test_ao3_fanon_end_to_end(tmp_path, monkeypatch, options):
    monkeypatch.setenv("FANDOM_SEARCH_WORKERS", "0")
    works = tmp_path / "works"
    works.mkdir()
    for name, text in TEXTS.items():
        (works / name).write_text(text, encoding="utf-8")
    script = tmp_path / "script.txt"
    script.write_text(SCRIPT, encoding="utf-8")
    prefix = str(tmp_path / "out")
    main(["fanon", str(works), str(script), "-o", prefix] + options)
    args = dict(length=8, min_works=2, max_share=100, keep_case=False, top=1000)
    for flag, key in (("--length", "length"), ("--min-works", "min_works"),
                      ("--max-share", "max_share"), ("--top", "top")):
        if flag in options:
            args[key] = int(options[options.index(flag) + 1])
    args["keep_case"] = "--keep-case" in options
    want = fr.tables(str(works), [str(script)], **args)
    assert len(want[0]) and len(want[1]) and len(want[2])
    for suffix, head, rows in zip(fr.SUFFIXES, fr.HEADS, want):
        assert fr.read_csv(prefix + suffix) == fr.csv_text(head, rows), suffix


@pytest.mark.parametrize("case, options, with_script", mfg.CASES)
def test_ao3_fanon_gives_the_committed_files(tmp_path, monkeypatch, case, options, with_script):
    monkeypatch.setenv("FANDOM_SEARCH_WORKERS", "0")
    monkeypatch.chdir(ROOT)
    prefix = str(tmp_path / "g")
    main(["fanon", mfg.WORKS] + ([mfg.SCRIPT] if with_script else []) + ["-o", prefix] + options)
    for suffix, name in zip(fr.SUFFIXES, mfg.golden_names(case)):
        assert fr.read_csv(prefix + suffix) == fr.read_csv(os.path.join(ROOT, "tests", "golden", name))
