"""`groups` on the GPU: fs_groups / fs_groups_rows against the restated contract
(tests/groups_restated.py), every field of every group, cell and word row compared for equality;
numbers of works in a group, of script words and of labels around every size the kernels treat
differently; `ao3.py groups` byte for byte against the oracle's three files."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, groups, synth
from fandom_search_amd.cli import main
from tests import groups_restated as gr
from tests.golden import make_groups_golden as mgg
from tests.test_gpu_pairs import from_spans, records

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# fs_groups.hip: works per slab of a group (a larger group is split over slabs whose partial
# depths meet in atomics); a lane takes 64 script words (one 64-bit coverage word), a wave
# 64 of them: a segment of lanes is the power of two above fewer words, else 64
SPLIT = 255
WORD = 64
SEGMENT = 64 * WORD


def lists(mem):
    """(mem_off, mem_grp) of a list of group lists."""
    off = np.zeros(len(mem) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in mem])
    return off, np.array([g for m in mem for g in m], dtype=np.uint32)


def oracle(cols, n_works, n_script, mem, n_groups, label_of, n_labels, m, g, k):
    recs = list(zip(*(c.tolist() for c in cols)))
    found = gr.groups(recs, n_works, n_script, [list(x) for x in mem], n_groups,
                      None if label_of is None else list(label_of), n_labels, m, g, k)
    out = []
    for part, dt, keys in zip(found, (abi.GROUP_DTYPE, abi.GROUP_CELL_DTYPE,
                                      abi.GROUP_WORD_DTYPE),
                              (gr.GROUP_KEYS, gr.CELL_KEYS, gr.WORD_KEYS)):
        a = np.zeros(len(part), dtype=dt)
        for name in keys:
            a[name] = [d[name] for d in part]
        out.append(a)
    return tuple(out)


def assert_equal(got, want):
    for a, b, dt in zip(got, want, (abi.GROUP_DTYPE, abi.GROUP_CELL_DTYPE, abi.GROUP_WORD_DTYPE)):
        assert len(a) == len(b), (dt.names[:2], len(a), len(b))
        for name in dt.names:                              # (the reserved words, 0, too)
            bad = np.nonzero(a[name] != b[name])[0]
            assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]])


def with_exact(cols, seed=0):
    exact = (np.random.default_rng(seed).random(len(cols[0])) < 0.6).astype(np.uint8)
    return tuple(cols) + (exact,)


def scenes(n_script, n_labels, seed=0):
    if not n_labels:
        return None
    cuts = np.sort(np.random.default_rng(seed).integers(0, max(1, n_script), size=n_labels - 1))
    return np.searchsorted(cuts, np.arange(n_script), side="right").astype(np.uint32)


def check(cols, n_works, n_script, mem, n_groups, n_labels=3, m=6, g=0, k=1):
    label_of = scenes(n_script, n_labels)
    off, grp = lists(mem)
    got = groups.find_groups(*cols, n_works, n_script, off, grp, n_groups, label_of, n_labels,
                             m, g, k)
    assert_equal(got, oracle(cols, n_works, n_script, mem, n_groups, label_of, n_labels, m, g, k))
    return got


def none_groups(n):
    a = np.zeros(n, dtype=abi.GROUP_DTYPE)
    a["peak_first"] = a["top_label"] = abi.FS_NONE
    return a


def test_no_records_one_record_no_works_no_groups():
    empty = (np.zeros(0, np.uint32),) * 3 + (np.zeros(0, np.uint8),)
    found = check(empty, 3, 10, [[0], [0, 1], []], 2)
    assert (found[0] == none_groups(2)).all() and not len(found[1]) and not len(found[2])
    found = check(empty, 0, 0, [], 0, n_labels=0)
    assert all(len(p) == 0 for p in found)
    found = check(empty, 0, 5, [], 4)                       # groups without works
    assert (found[0] == none_groups(4)).all()
    one = (np.array([1], np.uint32), np.array([7], np.uint32), np.array([9], np.uint32),
           np.array([1], np.uint8))
    found = check(one, 3, 10, [[0], [0, 2], []], 3, m=1)    # group 1 has no work
    assert found[0]["n_works"].tolist() == [1, 0, 1] and found[0]["covered"].tolist() == [1, 0, 1]
    assert found[2]["orig_ix"].tolist() == [9, 9] and found[1]["n_exact"].tolist() == [1, 1]
    found = check(one, 3, 10, [[0], [0, 2], []], 3, m=2)    # a record, no passage
    assert not found[0]["covered"].any() and found[0]["n_words"].tolist() == [1, 0, 1]
    found = check(one, 3, 10, [[], [], []], 3, m=1)         # works in no group
    assert (found[0] == none_groups(3)).all()
    found = check(one, 3, 10, [[0], [0], [0]], 1, m=1, n_labels=0)
    assert found[0]["top_label"].tolist() == [abi.FS_NONE] and not len(found[1])
    assert check(one, 3, 10, [[], [], []], 0, n_labels=0)[0].size == 0


@pytest.mark.parametrize("n_script", [1, 63, 64, 65, 4 * WORD - 1, 4 * WORD + 1, SEGMENT - WORD,
                                      SEGMENT - 1, SEGMENT, SEGMENT + 1, SEGMENT + WORD + 1])
def test_script_sizes_around_a_word_and_a_segment(n_script):
    sizes = np.random.default_rng(n_script).integers(0, 40, size=40)
    sizes[[3, 36]] = 5
    cols = with_exact(records(sizes, n_script, seed=n_script))
    for w in (3, 36):                                       # the last script word, twice
        cols[2][int(np.nonzero(cols[0] == w)[0][0])] = n_script - 1
    rng = np.random.default_rng(n_script + 1)
    mem = [sorted(rng.choice(7, size=int(rng.integers(0, 4)), replace=False).tolist()) + [7]
           for _ in range(40)]
    found = check(cols, 40, n_script, mem, 9, n_labels=min(n_script, 5), m=1)
    last = found[2][(found[2]["group"] == 7) & (found[2]["orig_ix"] == n_script - 1)]
    assert len(last) == 1 and last[0]["n_works"] >= 2
    if n_script > 1:
        check(cols, 40, n_script, mem, 9, n_labels=2, m=3, g=1, k=2)


@pytest.mark.parametrize("members", [1, 63, 64, 65, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT + 1])
def test_works_in_a_group_around_a_slab(members):
    n_script, n_works = 150, members + 2
    rng = np.random.default_rng(members)
    spans_of = [[(int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))
                 for _ in range(int(rng.integers(1, 3)))] for _ in range(n_works)]
    cols = with_exact(from_spans(spans_of), members)
    # group 1: `members` works; group 0 and 2: the works around them, which are in no other
    mem = [[0]] + [[1] + ([3] if w % 3 == 0 else []) for w in range(members)] + [[2]]
    found = check(cols, n_works, n_script, mem, 4, m=3)
    assert found[0]["n_passage_works"][1] == members
    check(cols, n_works, n_script, mem, 4, m=3, k=2, n_labels=70)


def test_one_group_of_all_of_a_thousand_works_and_a_thousand_groups_of_one():
    n_works, n_script = 1000, 300
    rng = np.random.default_rng(5)
    spans_of = [[(120, 8)] + [(int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))]
                for _ in range(n_works)]
    cols = with_exact(from_spans(spans_of), 5)
    found = check(cols, n_works, n_script, [[0]] * n_works, 1, m=3)
    assert found[0]["peak"][0] == 1000 and found[0]["n_works"][0] == 1000
    assert found[0]["peak_first"][0] <= 120
    found = check(cols, n_works, n_script, [[w] for w in range(n_works)], n_works, m=3)
    assert (found[0]["peak"] == 1).all() and (found[0]["n_passage_works"] == 1).all()
    check(cols, n_works, n_script, [[0]] * n_works, 1, m=3, k=1001)     # above every depth
    check(cols, n_works, n_script, [[0]] * n_works, 1, m=3, k=300)      # above a slab's count


@pytest.mark.parametrize("n_groups", [1023, 1025, 2049])
def test_groups_around_the_scan_s_chunk(n_groups):
    """k_groups_scan takes 1024 groups per chunk: every group has cells and word rows, so the
    offsets of the groups past a chunk carry the sums of the chunks in front."""
    n_script = 300
    rng = np.random.default_rng(n_groups)
    spans_of = [[(int(rng.integers(0, n_script - 12)), int(rng.integers(3, 13)))]
                for _ in range(n_groups)]
    cols = with_exact(from_spans(spans_of), n_groups)
    # work w is in group w, and every third one in the group after it as well
    mem = [sorted({w, (w + 1) % n_groups} if w % 3 == 0 else {w}) for w in range(n_groups)]
    found = check(cols, n_groups, n_script, mem, n_groups, m=3)
    assert (found[0]["n_passage_works"] >= 1).all() and (found[0]["covered"] >= 3).all()
    assert len(set(found[1]["group"].tolist())) == n_groups == len(set(found[2]["group"].tolist()))


@pytest.mark.parametrize("k", [1, 3])
def test_twenty_groups_per_work_out_of_three_hundred(k):
    n_works, n_script, n_groups = 400, 200, 300
    sizes = np.random.default_rng(20).integers(0, 40, size=n_works)
    cols = with_exact(records(sizes, n_script, seed=20), 20)
    rng = np.random.default_rng(21)
    p = 1.0 / np.arange(1, n_groups + 1)
    mem = [sorted(rng.choice(n_groups, size=20, replace=False, p=p / p.sum()).tolist())
           for _ in range(n_works)]
    found = check(cols, n_works, n_script, mem, n_groups, n_labels=7, m=3, k=k)
    assert found[0]["n_works"].max() > SPLIT and found[0]["n_works"].min() < 10
    assert len(found[2]) > 1000


def test_bridged_words_count_in_depth_and_a_repeated_line_counts_once():
    # work 0 steps over script words 3 and 4; work 1 repeats 0..5 ten times; work 2 covers 3..8
    f0 = [0, 1, 2, 5, 6, 7]
    work = [0] * 6 + [1] * 60 + [2] * 6
    fan = f0 + [20 * r + j for r in range(10) for j in range(6)] + list(range(6))
    orig = f0 + [j for r in range(10) for j in range(6)] + list(range(3, 9))
    cols = with_exact(tuple(np.array(c, dtype=np.uint32) for c in (work, fan, orig)))
    found = check(cols, 3, 9, [[0, 1], [0], [1]], 2, m=3, g=2)
    assert found[0]["n_words"].tolist() == [66, 12] and found[0]["covered"].tolist() == [8, 9]
    by = {(int(r["group"]), int(r["orig_ix"])): int(r["n_works"]) for r in found[2]}
    assert by[0, 3] == 2 and by[0, 4] == 2                  # bridged by work 0, read by work 1
    assert by[0, 0] == 2 and by[1, 3] == 2 and by[1, 8] == 1
    assert found[0]["n_passages"].tolist() == [11, 2]
    found = check(cols, 3, 9, [[0, 1], [0], [1]], 2, m=3, g=0)
    by = {(int(r["group"]), int(r["orig_ix"])): int(r["n_works"]) for r in found[2]}
    assert by[0, 3] == 1 and by[0, 4] == 1 and (1, 4) in by and found[0]["n_passages"][0] == 12


def _call(L, cols, n_works, n_script, off, grp, n_groups, m, k, out, caps, n, n_rows=None,
          label_of=None, n_labels=0):
    return L.fs_groups(0, abi.ptr(cols[0], C.c_uint32), abi.ptr(cols[1], C.c_uint32),
                       abi.ptr(cols[2], C.c_uint32), abi.ptr(cols[3], C.c_uint8),
                       len(cols[0]) if n_rows is None else n_rows, n_works, n_script,
                       abi.ptr(off, C.c_uint64), abi.ptr(grp, C.c_uint32), n_groups,
                       abi.ptr(label_of, C.c_uint32), n_labels, m, 0, k,
                       out[0].ctypes.data_as(C.c_void_p),
                       out[1].ctypes.data_as(C.c_void_p) if caps[0] else None, caps[0],
                       C.byref(n[0]),
                       out[2].ctypes.data_as(C.c_void_p) if caps[1] else None, caps[1],
                       C.byref(n[1]))


def test_capacity_too_small_together_and_one_at_a_time():
    sizes = np.random.default_rng(8).integers(0, 60, size=60)
    cols = [np.ascontiguousarray(c) for c in with_exact(records(sizes, 300, seed=8), 8)]
    rng = np.random.default_rng(9)
    mem = [sorted(rng.choice(6, size=2, replace=False).tolist()) for _ in range(60)]
    label_of = scenes(300, 4)
    want = oracle(cols, 60, 300, mem, 6, label_of, 4, 3, 0, 1)
    kc, kw = len(want[1]), len(want[2])
    assert kc > 10 and kw > 100
    off, grp = lists(mem)
    L = _lib.load()
    n = (C.c_uint64(0), C.c_uint64(0))
    for caps in ((kc - 1, kw - 1), (kc - 1, kw), (kc, kw - 1), (0, 0)):
        out = (np.zeros(6, abi.GROUP_DTYPE), np.zeros(kc, abi.GROUP_CELL_DTYPE),
               np.zeros(kw, abi.GROUP_WORD_DTYPE))
        rc = _call(L, cols, 60, 300, off, grp, 6, 3, 1, out, caps, n, label_of=label_of, n_labels=4)
        assert rc == abi.FS_E_CAPACITY and (n[0].value, n[1].value) == (kc, kw)
        assert_equal((out[0], want[1], want[2]), want)      # the groups are complete
        assert not out[1]["n_words"].any() and not out[2]["n_works"].any()   # nothing else written
    rc = _call(L, cols, 60, 300, off, grp, 6, 3, 1, out, (kc, kw), n, label_of=label_of, n_labels=4)
    assert rc == abi.FS_OK and (n[0].value, n[1].value) == (kc, kw)
    assert_equal(out, want)


def test_refusals():
    cols = with_exact(records([300, 500, 200], 1000, seed=9))
    mem = [[0], [0, 1], [1]]

    def refused(c=cols, n_works=3, n_script=1000, mem=mem, n_groups=2, m=6, k=1, label_of=None,
                n_labels=0, off=None, code=abi.FS_E_INVALID):
        o, g = lists(mem)
        with pytest.raises(_lib.FsError) as e:
            groups.find_groups(*c, n_works, n_script, o if off is None else off, g, n_groups,
                               label_of, n_labels, m, 0, k)
        assert e.value.code == code
    refused(m=0)
    refused(k=0)
    refused(n_works=2, mem=mem[:2])                        # a work >= n_works
    refused(n_script=int(cols[2].max()))                   # an orig_ix >= n_script
    fan = cols[1].copy()
    fan[700], fan[701] = fan[701] + 1, fan[700]
    refused((cols[0], fan, cols[2], cols[3]))              # unsorted records
    refused(n_groups=1)                                    # a group >= n_groups
    refused(mem=[[0], [1, 1], [1]])                        # not strictly ascending
    refused(mem=[[0], [1, 0], [1]])
    refused(label_of=np.full(1000, 2, np.uint32), n_labels=2)          # a label >= n_labels
    refused(off=np.array([1, 1, 3, 4], np.uint64))         # mem_off[0] != 0
    refused(off=np.array([0, 3, 2, 4], np.uint64))         # mem_off decreases
    refused(n_script=(1 << 19) + 1, code=abi.FS_E_UNSUPPORTED)
    L = _lib.load()
    n = (C.c_uint64(0), C.c_uint64(0))
    out = (np.zeros(2, abi.GROUP_DTYPE),) * 3
    off, grp = lists(mem)
    rc = _call(L, cols, 3, 1000, off, grp, 2, 6, 1, out, (0, 0), n, n_rows=1 << 32)
    assert rc == abi.FS_E_UNSUPPORTED                      # (refused before a record is read)
    check(cols, 3, 1000, mem, 2)                           # and the same columns are accepted


def test_tables_above_the_cap_are_refused_before_anything_is_allocated():
    """include/fandom_search.h lists what is counted.  A few records; the sizes alone exceed
    FS_GROUPS_MAX_BYTES: 21 846 groups x 4 096 labels x 12 bytes of (group, label) counters,
    and 16 385 coverage rows of 8 192 words of 8 bytes (one row above it, as in `pairs`)."""
    one = with_exact((np.arange(4, dtype=np.uint32), np.zeros(4, np.uint32),
                      np.arange(4, dtype=np.uint32)))
    n_groups = abi.FS_GROUPS_MAX_BYTES // (4096 * 12) + 1
    assert n_groups == 21846
    with pytest.raises(_lib.FsError) as e:
        groups.find_groups(*one, 4, 8, *lists([[0]] * 4), n_groups, np.zeros(8, np.uint32), 4096,
                           1, 0, 1)
    assert e.value.code == abi.FS_E_UNSUPPORTED and "more than" in str(e.value)
    n_works = abi.FS_GROUPS_MAX_BYTES // ((1 << 19) // 8) + 1
    assert n_works == 16385
    with pytest.raises(_lib.FsError) as e:
        groups.find_groups(*one, n_works, 1 << 19, *lists([[0]] * n_works), 1, None, 0, 1, 0, 1)
    assert e.value.code == abi.FS_E_UNSUPPORTED and "more than" in str(e.value)
    found = groups.find_groups(*one, n_works, 5000, *lists([[0]] * n_works), 1, None, 0, 1, 0, 1)
    assert found[0]["covered"][0] == 4                     # the same columns, accepted


# ---- host columns and device records are one path ---------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257])            # around the pack kernel's workgroup
def test_host_columns_equal_device_records_with_the_flags_in_comb(n, synth_base):
    """fs_groups packs its columns into fs_row records on the device, the exact flag as comb:
    the output equals, byte for byte, fs_groups_rows over the same records built on the host
    with lev = 7 and comb = 0.0 / 1.0, and with the same flags spelt -0.0 / NaN."""
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    script = synth.script_tokens(200)
    ix = ScriptIndex(script, [synth_base["words"][int(t)] for t in script], synth_base["emb"],
                     synth.lsh_normals(6))
    sizes = [n - n // 2, n // 2] if n > 1 else [1]
    work, fan, orig, exact = with_exact(records(sizes, len(script), seed=n), n)
    assert 0 < exact.sum() < n or n == 1
    mem = [[0, 1 + w] for w in range(len(sizes))]
    m_off, m_grp = lists(mem)
    label_of = scenes(len(script), 3)
    args = (len(sizes), m_off, m_grp, 3, label_of, 3, 2, 1, 1)
    host = groups.find_groups(work, fan, orig, exact, len(sizes), len(script), *args[1:])
    assert host[0]["n_words"][0] == n and host[0]["n_exact"][0] == exact.sum()
    for yes, no in ((0.0, 1.0), (-0.0, np.nan)):
        rows = np.zeros(n, dtype=abi.ROW_DTYPE)
        rows["work"], rows["fan_ix"], rows["orig_ix"], rows["lev"] = work, fan, orig, 7
        rows["dist"] = np.nan
        rows["comb"] = np.where(exact != 0, yes, no)
        buf = torch.from_numpy(rows.view(np.uint8)).cuda()
        torch_ready()
        dev = ix.groups_device(buf.data_ptr(), n, *args)
        for a, b in zip(host, dev):
            assert a.tobytes() == b.tobytes()
    ix.close()


# ---- after a real search ---------------------------------------------------------------

def test_device_rows_equal_host_columns_after_a_search(synth_base):
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    vocab, emb = synth_base["words"], synth_base["emb"]
    n_works, per, n = 120, 1500, 6
    script = synth.script_tokens(3000)
    tok, off = synth.corpus_tokens(n_works, per, script)
    ix = ScriptIndex(script, [vocab[int(t)] for t in script], emb, synth.lsh_normals(n))
    corpus = ix.corpus(tok, off, synth_base["chars"], synth_base["off"])
    cap = len(tok) // 4
    buf = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    n_rows, _ = ix.search_device(corpus, buf.data_ptr(), cap)
    rows = buf[:n_rows * 32].cpu().numpy().view(abi.ROW_DTYPE)
    cols = tuple(np.ascontiguousarray(rows[c]) for c in ("work", "fan_ix", "orig_ix"))
    cols += ((rows["comb"] <= 0).astype(np.uint8),)
    rng = np.random.default_rng(3)
    mem = [[0] + sorted(rng.choice(np.arange(1, 12), size=3, replace=False).tolist())
           for _ in range(n_works)]
    m_off, m_grp = lists(mem)
    label_of = scenes(len(script), 9)
    for g, k in ((0, 1), (1, 2)):
        dev = ix.groups_device(buf.data_ptr(), n_rows, n_works, m_off, m_grp, 12, label_of, 9,
                               n, g, k)
        host = groups.find_groups(*cols, n_works, len(script), m_off, m_grp, 12, label_of, 9,
                                  n, g, k)
        assert_equal(dev, host)
        assert_equal(host, oracle(cols, n_works, len(script), mem, 12, label_of, 9, n, g, k))
    assert host[0]["n_passage_works"][0] > 50 and len(host[2]) > 100
    # the caller's own device buffers, too small first
    kc, kw = len(host[1]), len(host[2])
    d = [torch.zeros(nb, dtype=torch.uint8, device="cuda") for nb in (12 * 64, kc * 24, kw * 16)]
    torch_ready()
    ptrs = tuple(t.data_ptr() for t in d)
    with pytest.raises(_lib.FsError) as e:
        ix.groups_device(buf.data_ptr(), n_rows, n_works, m_off, m_grp, 12, label_of, 9, n, 1, 2,
                         out_ptrs=ptrs, caps=(kc, kw - 1))
    assert e.value.code == abi.FS_E_CAPACITY and e.value.required == (kc, kw)
    assert (d[0].cpu().numpy().view(abi.GROUP_DTYPE) == host[0]).all()
    assert not d[2].cpu().numpy().any()
    assert ix.groups_device(buf.data_ptr(), n_rows, n_works, m_off, m_grp, 12, label_of, 9, n, 1,
                            2, out_ptrs=ptrs, caps=(kc, kw)) == (kc, kw)
    assert (d[1].cpu().numpy().view(abi.GROUP_CELL_DTYPE) == host[1]).all()
    assert (d[2].cpu().numpy().view(abi.GROUP_WORD_DTYPE) == host[2]).all()
    assert ix.groups_device(buf.data_ptr(), 0, n_works, m_off, m_grp, 12, label_of, 9, n, 1, 2,
                            out_ptrs=ptrs, caps=(kc, kw)) == (0, 0)
    assert (d[0].cpu().numpy().view(abi.GROUP_DTYPE) == none_groups(12)).all()
    corpus.close()
    ix.close()


# ---- the command ------------------------------------------------------------------------

def _run_command(tmp_path, src_path, meta_path, by, m, g, k, reader):
    prefix = str(tmp_path / "p")
    assert main(["groups", src_path, meta_path, "--by", by, "-o", prefix, "--min-words", str(m),
                 "--max-gap", str(g), "--min-works", str(k), "--reader", reader]) == 0
    return tuple(open(p, "rb").read() for p in groups.output_names(src_path, prefix))


@pytest.mark.parametrize("reader", ["device", "python"])
@pytest.mark.parametrize("case,src,m,g,by", mgg.CASES)
def test_command_on_golden_inputs(tmp_path, case, src, m, g, by, reader):
    meta_path = os.path.join(GOLDEN, mgg.META)
    got = _run_command(tmp_path, os.path.join(GOLDEN, src), meta_path, by, m, g, 1, reader)
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    with open(meta_path, newline="", encoding="utf-8") as fh:
        want = gr.groups_csv(text, fh.read(), by, m, g, 1)
    assert got == tuple(t.encode("utf-8") for t in want)
    for name, part in zip(mgg.golden_names(case, m, g, by), got):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_search_then_groups(tmp_path, monkeypatch, synth_base):
    from fandom_search_amd import search
    vocab = synth_base["words"]
    n_works, per = 40, 1500
    script = synth.script_tokens(3000)
    fandir = tmp_path / "fanworks"
    synth.write_corpus(str(fandir), n_works, per, script, vocab)
    (tmp_path / "script.txt").write_text(synth.script_markup(script, vocab))
    names = sorted(os.listdir(str(fandir)))
    import csv
    import json
    with open(str(tmp_path / "meta.csv"), "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh)
        w.writerow(groups.META_FIELDS)
        for j, name in enumerate(names[:-2]):               # two works without metadata
            tags = {"Rating": "R%d" % (j % 3), "Additional Tags": "Fluff; T%d; T%d" % (j % 5, j % 7)}
            w.writerow([os.path.splitext(name)[0] + ".html", "t", "a%d" % (j % 4), "s", "",
                        "%d-0%d-11" % (2015 + j % 3, 1 + j % 9), "English", json.dumps(tags)])
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    monkeypatch.delenv("FANDOM_SEARCH_VECTORS", raising=False)
    assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--synthetic-vocab"]) == 0
    dated = "match-6gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    with open(dated, newline="", encoding="utf-8") as fh:
        text = fh.read()
    with open("meta.csv", newline="", encoding="utf-8") as fh:
        meta = fh.read()
    for by, k in (("tag", 2), ("month", 1)):
        assert main(["groups", dated, "meta.csv", "--by", by, "--min-works", str(k)]) == 0
        want = gr.groups_csv(text, meta, by, min_works=k)   # default prefix: beside the input
        for path, part in zip(groups.output_names(dated), want):
            with open(path, "rb") as fh:
                assert fh.read() == part.encode("utf-8"), path
        assert want[2].count("\r\n") > 10 and "(no metadata)" in want[0]
