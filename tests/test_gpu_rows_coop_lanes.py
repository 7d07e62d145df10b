"""The k_scan_rows instance that ends in k_compact (searches overlapped on several lanes) under
the switches of the shared rounds.  That instance does all rounds of a range in the range's own
wave (with the slices it does not fit its 96 registers), so FS_ROWS_COOP and
FS_ROWS_XPOOL must not change its output by a byte, and its launch must not touch the slices'
LDS, which it does not hold.

The corpus is the small one of test_scan_rows_and_chain_agree (test_gpu_parity.py): the
smallest shapes at which slices exist (quotes of 90, 150 and 300 tokens: one, two and five
slices per wave range), a range boundary falls inside a quote, and hits sit at work and range
boundaries."""
import os

import numpy as np
import pytest

from fandom_search_amd import abi, synth

from tests import util

pytestmark = pytest.mark.gpu

SWITCHES = ("FS_SCAN_ROWS", "FS_RANGES_CAPROW", "FS_LANES", "FS_ROWS_DISP_LDS", "FS_ROWS_COOP",
            "FS_ROWS_XPOOL", "FS_DIAG", "FS_ROWS_FINISH", "FS_ROWS_SHARES")
FORMS = ((False, 32), (True, 16), (8, 8))          # fs_row, 16-byte and 8-byte wire records
DENSE_WORK, DENSE_LEN = 3, 1400


class _Env:
    """The FS_* switches of one index, set while it is created (they are read there)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _corpus(n, V, script, first_work=0):
    lengths = [1500] * 40 + [0, 5, n, n - 1, 3000, 511, 512, 513]
    parts = [synth.fanwork_tokens(first_work + i, L, script, V) if L else np.zeros(0, np.uint32)
             for i, L in enumerate(lengths)]
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p) for p in parts])
    tok = np.concatenate(parts).astype(np.uint32)
    d0 = int(off[DENSE_WORK])
    tok[d0:d0 + DENSE_LEN] = script[100 + first_work:100 + first_work + DENSE_LEN]   # dense: every window a hit
    tok[int(off[7]) + 1490:int(off[7]) + 1500] = script[40:50]  # hit at the end of a work ...
    tok[int(off[8]):int(off[8]) + 10] = script[40:50]           # ... and at the start of the next
    for k in range(9, 30):                                      # hits straddling 512-token borders
        at = (int(off[k]) // 512 + 1) * 512 - (k % (n + 3))
        tok[at:at + n + 2] = script[700 + k:700 + k + n + 2]
    # quotes of 90, 150 and 300 tokens: one, two and five slices per wave range; one across a
    # 512-token border
    for k, (ln, where) in enumerate(((90, 200), (150, 300), (300, 100), (150, 450))):
        at = (int(off[31 + k]) // 512 + 1) * 512 + where
        tok[at:at + ln] = script[2000 + 400 * k:2000 + 400 * k + ln]
    return tok, off


def _setup(n, synth_base):
    from fandom_search_amd.vocab import pack_strings
    if n <= 6:
        words, emb, V = synth_base["words"], synth_base["emb"], synth.VOCAB_SIZE
        chars, coff = synth_base["chars"], synth_base["off"]
    else:
        V = 256
        words = synth.vocab_words(V)
        emb = np.eye(V, synth.EMB_DIM, dtype=np.float32)
        chars, coff = pack_strings(words)
    script = synth.script_tokens(5000, vocab_size=V)
    return dict(n=n, words=words, emb=emb, chars=chars, coff=coff, script=script,
                swords=[words[int(t)] for t in script], normals=synth.lsh_normals(n),
                cfg=abi.make_config(window_size=n))


def _index(S, env):
    from fandom_search_amd.engine import ScriptIndex
    with _Env(env):
        ix = ScriptIndex(S["script"], S["swords"], S["emb"], S["normals"], cfg=S["cfg"])
    assert ix.info["path"] == abi.FS_MODE_EXACT
    return ix


def _device_bytes(ix, c, cap):
    """The device buffer of a search in each record form, as it lies there: the header's count
    and the records, unsorted."""
    import torch
    out = []
    for packed, size in FORMS:
        buf = torch.zeros(32 + cap * size, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nw, _ = ix.search_end(ix.search_begin(c, buf.data_ptr(), cap, packed=packed, header=True))
        host = buf.cpu().numpy()
        assert int(host[:8].view(np.uint64)[0]) == nw
        out.append(host[:32 + nw * size].tobytes())
    return out


def _run(S, env, tok, off):
    ix = _index(S, env)
    c = ix.corpus(tok, off, S["chars"], S["coff"])
    rows, st = ix.search(c)
    res = dict(rows=rows, matches=st.matches, n=st.rows, dev=_device_bytes(ix, c, len(rows) + 3))
    ix.close()
    return res


_CACHE = {}


def _reference(n, synth_base):
    """Per n, once: the corpus, the chained kernels' and the oracle's rows, and the device
    buffers of four lanes without shared rounds."""
    if n not in _CACHE:
        S = _setup(n, synth_base)
        tok, off = _corpus(n, 256 if n > 6 else synth.VOCAB_SIZE, S["script"])
        chain = _run(S, {"FS_SCAN_ROWS": "0"}, tok, off)
        oi = util.oracle_index(S["cfg"], S["script"], S["words"], S["emb"], S["normals"])
        want, ost = oi.search(tok, off, S["chars"], S["coff"])
        oi.close()
        assert len(want) > DENSE_LEN
        util.assert_rows_equal(chain["rows"], want)
        plain = _run(S, {"FS_LANES": "4", "FS_ROWS_COOP": "0"}, tok, off)
        _CACHE[n] = dict(S=S, tok=tok, off=off, chain=chain, want=want, want_matches=ost.matches, plain=plain)
    return _CACHE[n]


VARIANTS = {
    "lanes4": {"FS_LANES": "4"},
    "caprow2": {"FS_LANES": "4", "FS_RANGES_CAPROW": "2"},
    "xpool8": {"FS_LANES": "4", "FS_ROWS_XPOOL": "8"},
    "xpool8_caprow2": {"FS_LANES": "4", "FS_ROWS_XPOOL": "8", "FS_RANGES_CAPROW": "2"},
    "lanes2": {"FS_LANES": "2"},
    "disp_mem": {"FS_LANES": "4", "FS_ROWS_DISP_LDS": "0"},
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("n", [6, 2, 8])
def test_several_lanes_keep_the_bytes(synth_base, n, variant):
    """Several lanes against the chained kernels (FS_SCAN_ROWS=0) and the C
    oracle, record for record, in all three record forms; and the device buffer, unsorted and
    with its header count, against the same search with FS_ROWS_COOP=0, byte for byte -- also
    when the staging rows, the slices' pool or both start far too small (the search reports
    what it needs and is repeated), on two lanes, and with the seeds read from memory."""
    ref = _reference(n, synth_base)
    got = _run(ref["S"], VARIANTS[variant], ref["tok"], ref["off"])
    util.assert_rows_equal(got["rows"], ref["chain"]["rows"])
    util.assert_rows_equal(got["rows"], ref["want"])
    assert got["matches"] == ref["want_matches"] == ref["chain"]["matches"]
    assert got["n"] == ref["chain"]["n"]
    for form, a, b, ch in zip(FORMS, got["dev"], ref["plain"]["dev"], ref["chain"]["dev"]):
        assert a == b, ("device buffer differs from FS_ROWS_COOP=0", form)
        assert a == ch, ("device buffer differs from the chained kernels", form)


def test_overlapped_searches_on_four_lanes(synth_base):
    """Four lanes, eight searches begun before any is ended, over two distinct corpora into
    distinct buffers: every buffer equals its synchronous result."""
    import torch
    ref = _reference(6, synth_base)
    S = ref["S"]
    tok2, off2 = _corpus(6, synth.VOCAB_SIZE, S["script"], first_work=100)
    ix = _index(S, {"FS_LANES": "4"})
    corpora = [ix.corpus(ref["tok"], ref["off"], S["chars"], S["coff"]),
               ix.corpus(tok2, off2, S["chars"], S["coff"])]
    sync = [ix.search(c)[0] for c in corpora]
    util.assert_rows_equal(sync[0], ref["want"])
    assert len(sync[1]) > DENSE_LEN and sync[1].tobytes() != sync[0].tobytes()
    cap = max(len(r) for r in sync) + 3
    bufs = [torch.zeros(32 + cap * 32, dtype=torch.uint8, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    tickets = []
    for i in range(8):
        try:
            tickets.append(ix.search_begin(corpora[i % 2], bufs[i].data_ptr(), cap, header=True))
        except Exception:
            # (an index holds a fixed number of searches in flight: end the oldest, go on)
            assert len(tickets) >= 4
            break
    begun = len(tickets)
    counts = [ix.search_end(t)[0] for t in tickets]
    for i in range(begun, 8):
        counts.append(ix.search_end(ix.search_begin(corpora[i % 2], bufs[i].data_ptr(), cap, header=True))[0])
    for i in range(8):
        host = bufs[i].cpu().numpy()
        want = sync[i % 2]
        assert counts[i] == len(want) and int(host[:8].view(np.uint64)[0]) == len(want)
        assert host[32:32 + 32 * len(want)].tobytes() == want.tobytes(), i
    ix.close()
