"""Several scripts over one fan corpus: a view of another index's corpus (fs_corpus_view,
ScriptIndex.corpus_view) searches the base's batch without a second upload, and must give
what a corpus of its own index over the same host buffers gives, byte for byte, batch after
batch of the base; `ao3.py search dir s1 s2 s3` must write, per script, the files a run with
that script alone writes."""

import glob
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, search, synth
from fandom_search_amd.vocab import pack_strings
from tests import util

pytestmark = pytest.mark.gpu

ROWS = 6000


def _clustered(seed=3, clusters=1024, per=8, noise=0.25):
    """Near-synonym table (unit vectors in tight clusters): LSH pipeline with component prefilters."""
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((clusters, 300))
    emb = np.repeat(centers, per, axis=0) + noise * rng.standard_normal((clusters * per, 300))
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    perm = rng.permutation(len(emb))
    out = np.empty_like(emb)
    out[perm] = emb
    return np.ascontiguousarray(out, dtype=np.float32), perm, np.argsort(perm)


def _case(kind, with_str):
    """(emb, script A, script B, script words of each, strings, batches): three batches of
    different sizes, each (tok_vec, work_off, tok_str or None)."""
    rng = np.random.default_rng(21)
    sizes = [(30, 700), (90, 900), (12, 400)]           # the second grows d_tok, the third shrinks
    if kind == "realistic":
        emb, group = synth.realistic_table(rows=ROWS)
        strings, vid = synth.realistic_vector_ids(ROWS)
        sa = synth._draw(np.random.default_rng(77), 3000, ROWS)
        sb = synth._draw(np.random.default_rng(78), 2500, ROWS)
        batches = []
        for i, (w, t) in enumerate(sizes):
            both = np.concatenate([sa[:1500], sb[:1500]])
            tok_str, off = synth.realistic_corpus(w, t, both, group, ROWS, seed=5 + i, first_work=100 * i,
                                                  oov_rate=0.05 if with_str else 0.0,
                                                  cap_rate=0.06 if with_str else 0.0)
            batches.append((vid[tok_str], off, tok_str if with_str else None))
        words_a = [strings[int(t)] for t in sa]
        words_b = [strings[int(t)] for t in sb]
        return emb, sa, sb, words_a, words_b, strings, batches
    words = synth.vocab_words()
    if kind == "exact":
        emb = synth.embedding()
        perm = inv = None
    else:
        emb, perm, inv = _clustered()
    sa = synth.script_tokens(3000, seed=101)
    sb = synth.script_tokens(2500, seed=202)
    strings = words + [w.upper() for w in words]
    batches = []
    for i, (w, t) in enumerate(sizes):
        ta, off = synth.corpus_tokens(w, t, sa, first_work=1000 * i)
        tb, _ = synth.corpus_tokens(w, t, sb, first_work=1000 * i + 500)
        tok = np.where(np.arange(len(ta)) % (2 * t) < t, ta, tb).astype(np.uint32)
        if perm is not None:                            # near-synonyms in place of a tenth of the tokens
            sel = np.nonzero(rng.random(len(tok)) < 0.1)[0]
            tok[sel] = perm[(inv[tok[sel]] // 8) * 8 + rng.integers(0, 8, size=len(sel))].astype(np.uint32)
        tok_str = None
        if with_str:                                    # capitalised strings of the same vectors
            tok_str = tok.copy()
            up = rng.random(len(tok)) < 0.05
            tok_str[up] += np.uint32(len(words))
        batches.append((tok, off, tok_str))
    words_a = [words[int(t)] for t in sa]
    words_b = [words[int(t)].upper() if i % 13 == 0 else words[int(t)] for i, t in enumerate(sb)]
    return emb, sa, sb, words_a, words_b, strings, batches


def _indexes(emb, sa, sb, words_a, words_b, **cfg_kw):
    from fandom_search_amd.engine import ScriptIndex
    normals = synth.lsh_normals(6)
    a = ScriptIndex(sa, words_a, emb, normals, cfg=abi.make_config(**cfg_kw))
    b = ScriptIndex(sb, words_b, emb, normals, cfg=abi.make_config(**cfg_kw))
    return a, b


def _device_rows(ix, corpus_list, packed, cap):
    """Searches of every corpus of `corpus_list` in flight together (search_begin ... then the
    search_ends), records to device buffers; returns [(bytes, stats)]."""
    import torch
    from fandom_search_amd.engine import torch_ready
    rec = 32 if not packed else packed
    bufs = [torch.zeros(cap * rec, dtype=torch.uint8, device="cuda") for _ in corpus_list]
    torch_ready()
    tickets = [ix.search_begin(c, b.data_ptr(), cap, packed=packed) for c, b in zip(corpus_list, bufs)]
    out = []
    for t, b in zip(tickets, bufs):
        n, st = ix.search_end(t)
        out.append((b[:n * rec].cpu().numpy().tobytes(), st))
    return out


@pytest.mark.parametrize("with_str", [False, True])
@pytest.mark.parametrize("kind", ["exact", "synonyms", "realistic"])
def test_view_equals_own_corpus_over_three_batches(kind, with_str):
    emb, sa, sb, words_a, words_b, strings, batches = _case(kind, with_str)
    chars, coff = pack_strings(strings)
    a, b = _indexes(emb, sa, sb, words_a, words_b)
    tok, off, tstr = batches[0]
    base = a.corpus(tok, off, chars, coff, tok_str=tstr)
    view = b.corpus_view(base)
    try:
        paths = set()
        for i, (tok, off, tstr) in enumerate(batches):
            if i:
                base.update_begin(tok, off, tok_str=tstr)
                base.update_end()
            own = b.corpus(tok, off, chars, coff, tok_str=tstr)
            want, sw = b.search(own)
            got, sg = b.search(view)
            util.assert_rows_equal(got, want)
            assert len(want) > 0
            assert sg.windows_processed == sw.windows_processed > 0
            assert sg.path == sw.path and b.kernel_name(view) == b.kernel_name(own)
            assert sg.handoff_fallbacks == 0 and sw.handoff_fallbacks == 0
            paths.add(sg.path)
            # the base's own index still searches its batch
            _, sa_st = a.search(base)
            assert sa_st.handoff_fallbacks == 0 and sa_st.windows_processed == sw.windows_processed
            # two searches in flight on B, rows on the device
            modes = [False]
            if sg.path == abi.FS_MODE_EXACT:
                modes.append(8)
            for packed in modes:
                (gb, gs), (wb, ws) = _device_rows(b, [view, own], packed, max(1024, len(want) + 64))
                assert gb == wb and len(gb) > 0
                assert gs.handoff_fallbacks == 0 and ws.handoff_fallbacks == 0
                assert gs.windows_processed == ws.windows_processed
            own.close()
        assert paths == {abi.FS_MODE_EXACT if kind == "exact" else abi.FS_MODE_GENERAL}
        if kind == "synonyms":
            assert b.component_sizes()[1]             # the component prefilters were in use
        if kind == "realistic":
            assert b.share_info()["flags"] & 32       # the share rule was in use
    finally:
        view.close()
        base.close()
        a.close()
        b.close()


def test_update_refused_while_a_view_searches_and_lifetimes():
    import torch
    from fandom_search_amd.engine import ScriptIndex, torch_ready
    emb, sa, sb, words_a, words_b, strings, batches = _case("exact", False)
    chars, coff = pack_strings(strings)
    a, b = _indexes(emb, sa, sb, words_a, words_b)
    tok, off, _ = batches[0]
    base = a.corpus(tok, off, chars, coff)
    view = b.corpus_view(base)
    own = b.corpus(tok, off, chars, coff)
    want, _ = b.search(own)
    L = _lib.load()
    cap = len(want) + 64
    buf = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    torch_ready()
    t = b.search_begin(view, buf.data_ptr(), cap)
    tok1, off1, _ = batches[1]
    tok1 = abi.as_u32(tok1)
    off1 = abi.as_u64(off1)
    rc = L.fs_corpus_update_begin(base._h, abi.ptr(tok1, abi.C.c_uint32), None,
                                  abi.ptr(off1, abi.C.c_uint64), len(off1) - 1)
    assert rc == abi.FS_E_INVALID
    assert b"view" in L.fs_last_error() and b"in flight" in L.fs_last_error()
    n, st = b.search_end(t)
    got = np.frombuffer(buf[:n * 32].cpu().numpy().tobytes(), dtype=abi.ROW_DTYPE)
    util.assert_rows_equal(got, want)
    assert st.handoff_fallbacks == 0
    # a view is updated through its base only
    assert L.fs_corpus_update_begin(view._h, abi.ptr(tok1, abi.C.c_uint32), None,
                                    abi.ptr(off1, abi.C.c_uint64), len(off1) - 1) == abi.FS_E_INVALID
    assert L.fs_corpus_update_end(view._h) == abi.FS_E_INVALID
    with pytest.raises(ValueError):
        view.update_begin(tok1, off1)
    # views that do not fit the base are refused, each with its reason
    normals6 = synth.lsh_normals(6)
    for ix, what in ((ScriptIndex(sb, words_b, emb, synth.lsh_normals(7), cfg=abi.make_config(window_size=7)),
                      b"window size"),
                     (ScriptIndex(sb, words_b, np.vstack([emb, emb[:10]]), normals6, cfg=abi.make_config()),
                      b"vector count"),
                     (a, b"belongs to this index")):
        with pytest.raises(_lib.FsError) as e:
            ix.corpus_view(base)
        assert e.value.code == abi.FS_E_INVALID and what in L.fs_last_error(), L.fs_last_error()
        if ix is not a:
            ix.close()
    with pytest.raises(TypeError):
        a.corpus_view(view)                           # (a view is no base)
    h = abi.C.c_void_p()
    assert L.fs_corpus_view(a._h, view._h, abi.C.byref(h)) == abi.FS_E_INVALID and not h.value
    assert b"not a view" in L.fs_last_error()
    # the base goes first: the view is detached and can only be destroyed
    base._views.discard(view)
    base.close()
    rc = L.fs_search_corpus(b._h, view._h, want.ctypes.data_as(abi.C.c_void_p), len(want), 0,
                            abi.C.byref(abi.C.c_uint64()), None)
    assert rc == abi.FS_E_INVALID and b"destroyed" in L.fs_last_error()
    assert b.kernel_name(view) == ""
    view.close()
    view.close()
    # the index B still searches its own corpora
    again, st = b.search(own)
    util.assert_rows_equal(again, want)
    own.close()
    a.close()
    b.close()


# ---- the command end to end -----------------------------------------------------------------

N_WORKS = 1250


def _write_inputs(tmp_path, words, vocab_size):
    """Three scripts and N_WORKS small works, each quoting one of them."""
    scripts = [synth.script_tokens(1200, vocab_size=vocab_size, seed=300 + k) for k in range(3)]
    paths = []
    sdir = tmp_path / "scripts"
    sdir.mkdir()
    for k, sc in enumerate(scripts):
        p = sdir / ("script-%d.txt" % k)
        p.write_text(synth.script_markup(sc, words))
        paths.append(str(p))
    fan = tmp_path / "fan"
    fan.mkdir()
    for i in range(N_WORKS):
        tok = synth.fanwork_tokens(i, 160, scripts[i % 3], vocab_size)
        (fan / synth.work_name(i)).write_text(" ".join(words[int(t)] for t in tok))
    return str(fan), paths


def _outputs(d):
    batches = sorted(glob.glob(os.path.join(d, "match-6gram-batch-*.csv")))
    dated = sorted(set(glob.glob(os.path.join(d, "match-6gram-*.csv"))) - set(batches))
    assert len(dated) == 1, dated
    with open(dated[0], "rb") as fh:
        body = fh.read()
    return {os.path.basename(p): open(p, "rb").read() for p in batches}, body


def _run(argv, capsys):
    from fandom_search_amd.cli import main
    search.set_vocab(None)
    try:
        assert main(argv) == 0
    finally:
        search.set_vocab(None)
    return capsys.readouterr().out


@pytest.mark.parametrize("table", ["synthetic", "realistic"])
def test_cli_several_scripts_write_what_single_runs_write(tmp_path, monkeypatch, capsys, table):
    if table == "synthetic":
        words = synth.vocab_words()
        fan, scripts = _write_inputs(tmp_path, words, len(words))
        extra = ["--synthetic-vocab"]
        monkeypatch.setenv("FANDOM_SEARCH_SYNTHETIC_VOCAB", "1")
    else:
        emb, _ = synth.realistic_table(rows=ROWS)
        words = synth.realistic_words(ROWS)
        np.savez(tmp_path / "vectors.npz", words=np.array(words), vectors=emb)
        fan, scripts = _write_inputs(tmp_path, words, ROWS)
        extra = ["--vectors", str(tmp_path / "vectors.npz")]
        monkeypatch.setenv("FANDOM_SEARCH_VECTORS", str(tmp_path / "vectors.npz"))
        monkeypatch.delenv("FANDOM_SEARCH_SYNTHETIC_VOCAB", raising=False)
    window = ["-s", "40", "-n", "1150"]                # three clusters: 500, 500, 150
    monkeypatch.chdir(tmp_path)
    out = _run(["search", fan] + scripts + window + extra + ["--out-dir", str(tmp_path / "multi")], capsys)
    assert out.count("Processing cluster") == 3, out
    assert not glob.glob(str(tmp_path / "match-*.csv"))
    n_rows = 0
    for k, sc in enumerate(scripts):
        single = tmp_path / ("single-%d" % k)
        out1 = _run(["search", fan, sc] + window + extra + ["--out-dir", str(single)], capsys)
        assert out1.count("Processing cluster") == 3
        want_batches, want_dated = _outputs(str(single))
        got_batches, got_dated = _outputs(str(tmp_path / "multi" / ("script-%d" % k)))
        assert sorted(got_batches) == ["match-6gram-batch-%d.csv" % i for i in range(3)]
        assert got_batches == want_batches
        assert got_dated == want_dated
        n_rows += want_dated.count(b"\n") - 1
    assert n_rows > 100                                 # (the works quote the scripts)
