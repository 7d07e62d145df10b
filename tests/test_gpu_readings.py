"""`ao3.py readings` on the GPU: fs_readings against its plain-Python restatement
(tests/readings_restated.py), equality of all three counts, every fs_reading and every
fs_reading_span, with the sequence hash whole, cut to 4 bits and cut to nothing; and the command
under both readers against the committed expected CSVs."""

import ctypes as C
import datetime
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, readings
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests import readings_restated as rr
from tests.golden import make_readings_golden as mrg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BITS = [None, "4", "0"]     # FS_READINGS_HASH_BITS: the default, 16 hashes, every passage collides
FAN_GAP = 10                # fan words between two quotations of a work: they never join


@pytest.fixture(params=BITS, ids=lambda b: "bits_%s" % b)
def bits(request, monkeypatch):
    set_bits(monkeypatch, request.param)
    return request.param


def set_bits(monkeypatch, value):
    if value is None:
        monkeypatch.delenv("FS_READINGS_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("FS_READINGS_HASH_BITS", value)


def layout(quotes):
    """Columns (work, fan_ix, orig_ix, spell), sorted by (work, fan_ix), of the quotations
    (work, orig_first, spells[, skipped positions]) laid out one behind another in their work."""
    cols = [[], [], [], []]
    at = {}
    for q in sorted(quotes, key=lambda q: q[0]):            # stable
        work, orig, spells = q[:3]
        skip = q[3] if len(q) > 3 else ()
        fan, k = at.get(work, 0), 0
        for j in range(len(spells) + len(skip)):
            if j not in skip:
                for c, v in zip(cols, (work, fan + j, orig + j, spells[k])):
                    c.append(v)
                k += 1
        at[work] = fan + len(spells) + len(skip) + FAN_GAP
    return [np.asarray(c, dtype=np.uint32) for c in cols]


def check(cols, n_works, n_script, n_spell, min_words=6, max_gap=0):
    """fs_readings against the restatement; returns (readings, spans, passages)."""
    found, spans, n_pass = readings.find_readings(*cols, n_works, n_script, n_spell, min_words,
                                                  max_gap)
    want_r, want_s, want_n = rr.readings(list(zip(*(c.tolist() for c in cols))), n_works, n_script,
                                         n_spell, min_words, max_gap)
    assert (n_pass, len(found), len(spans)) == (want_n, len(want_r), len(want_s))
    assert found.dtype == abi.READING_DTYPE and spans.dtype == abi.READING_SPAN_DTYPE
    assert [tuple(s) for s in spans.tolist()] == [tuple(s[k] for k in rr.SPAN_KEYS) for s in want_s]
    assert [tuple(r) for r in found.tolist()] == [tuple(r[k] for k in rr.READING_KEYS) for r in want_r]
    return found, spans, n_pass


def line(k, length=6, n_spell=1000):
    """Spellings of a line that differs from every other line(k') in each word."""
    return [(k * 31 + j * 7) % n_spell for j in range(length)]


# ---- small inputs ----------------------------------------------------------------------------

def test_zero_records_one_record_one_passage(bits):
    none = [np.zeros(0, dtype=np.uint32)] * 4
    assert [len(x) for x in check(none, 0, 3, 0)[:2]] == [0, 0]
    one = [np.asarray([v], dtype=np.uint32) for v in (4, 9, 2, 6)]
    found, spans, n = check(one, 5, 3, 7, min_words=1)
    assert found.tolist() == [(0, 2, 2, 1, 1, 1, 0, 1, 0)] and spans.tolist() == [(2, 2, 1, 1, 1, 0)]
    assert check(one, 5, 3, 7, min_words=2)[2] == 0
    found, _, n = check(layout([(0, 10, line(1))]), 1, 20, 1000)
    assert n == 1 and found.tolist() == [(0, 10, 15, 6, 1, 1, 0, 1, 0)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_passage_counts_all_distinct_and_all_one_reading(bits, n):
    # one span: the last word tells the readings apart, and they tie on works and passages
    distinct = layout([(k % 7, 5, [1, 2, 3, 4, 5, 10 + (n - k)]) for k in range(n)])
    found, spans, _ = check(distinct, 7, 20, n + 11)
    assert len(found) == n and len(spans) == 1 and found["rank"].tolist() == list(range(1, n + 1))
    found, spans, _ = check(layout([(k % 7, 5, line(3)) for k in range(n)]), 7, 20, 1000)
    assert found["n_passages"].tolist() == [n] and found["n_works"].tolist() == [min(n, 7)]
    # every span its own, in script order whatever the order of the works
    check(layout([(k % 5, (k * 37) % 5000, line(0)) for k in range(n)]), 5, 5010, 1000)


def test_passage_lengths_in_one_input(bits):
    lengths = (1, 6, 63, 64, 65, 129, 1000)
    quotes = []
    for w in range(3):
        for k, length in enumerate(lengths):
            spells = [(j * 13 + k) % 50 for j in range(length)]
            if w == 2:
                spells[-1] = 49 - spells[-1]                  # the last record of any length
            quotes.append((w, 100 * k, spells))
    found, spans, n = check(layout(quotes), 3, 2000, 50, min_words=1)
    assert n == 21 and len(spans) == 7 and len(found) == 14
    assert sorted(set(found["n_words"].tolist())) == list(lengths)


@pytest.mark.parametrize("length", [6, 64, 65, 200])
def test_pairs_that_differ_in_one_place(bits, length):
    base = [j % 9 for j in range(length)]
    last, first = list(base), list(base)
    last[-1] = 9
    first[0] = 9
    quotes = [(0, 50, base), (1, 50, last), (2, 50, first), (3, 51, base), (4, 50, base),
              (5, 50, base[:-1]), (6, 50, base + [3])]
    found, spans, n = check(layout(quotes), 7, 400, 10, min_words=5)
    assert n == 7 and len(found) == 6 and len(spans) == 4
    # one bridged offset: the same span, length and spellings
    gaps = [(0, 50, base, (2,)), (1, 50, base, (3,)), (2, 50, base, (2, 3)), (3, 50, base, (3, 4)),
            (4, 50, base, (length - 1,)), (5, 50, base, (2,))]
    found, spans, n = check(layout(gaps), 6, 400, 10, min_words=5, max_gap=2)
    assert n == 6 and len(found) == 5
    assert [s[:2] for s in spans.tolist()] == [(50, 50 + length), (50, 51 + length)]


def test_ranking_ties_at_every_level(bits):
    a, b, c, d, e = ([1, 2, 3, 4, 5, k] for k in range(5))
    quotes = [(0, 9, e),                                      # 1 work, 1 passage, first of all
              (1, 9, a), (2, 9, a),                           # 2 works, 2 passages
              (1, 9, b), (2, 9, b),                           # ... the same: later first record
              (3, 9, c), (3, 9, c), (3, 9, c),                # 1 work, 3 passages
              (4, 9, d), (5, 9, d), (5, 9, d)]                # 2 works, 3 passages
    found, spans, _ = check(layout(quotes), 6, 20, 6)
    assert [(r[4], r[5]) for r in found.tolist()] == [(3, 2), (2, 2), (2, 2), (3, 1), (1, 1)]
    assert found["first"].tolist() == [48, 6, 12, 30, 0]
    assert spans.tolist() == [(9, 14, 11, 6, 5, 0)]


def test_one_work_with_ten_passages_beside_ten_works_with_one(bits):
    quotes = [(0, 9, line(1))] * 10 + [(w, 9, line(2)) for w in range(1, 11)]
    found, spans, _ = check(layout(quotes), 11, 20, 1000)
    assert [(r[4], r[5]) for r in found.tolist()] == [(10, 10), (10, 1)]


def test_a_span_whose_readings_share_works(bits):
    quotes = [(w, 9, line(k)) for w in range(4) for k in range(3)] + [(4, 9, line(0))]
    found, spans, _ = check(layout(quotes), 5, 20, 1000)
    assert spans.tolist() == [(9, 14, 13, 5, 3, 0)] and found["n_works"].sum() == 13


# ---- random inputs ---------------------------------------------------------------------------

def random_records(rng, n, n_works, n_script, n_spell, starts):
    """Records whose runs start at one of `starts` (skewed), mostly spelt as the script word
    decides: many repeated readings and many unique ones."""
    work = np.sort(rng.integers(0, n_works, n)).astype(np.int64)
    cut = rng.random(n) < 0.125
    cut[0] = True
    cut[1:] |= work[1:] != work[:-1]
    start = starts[(rng.random(n) ** 3 * len(starts)).astype(np.int64)]
    head = np.maximum.accumulate(np.where(cut, np.arange(n), 0))
    orig = start[head] + (np.arange(n) - head)
    over = orig >= n_script                                   # wraps: a break in the run
    orig = np.where(over, orig % n_script, orig)
    fan = np.arange(n) + np.cumsum(cut) * 3
    fan -= np.concatenate([[0], fan[:-1]])[np.maximum.accumulate(
        np.where(np.concatenate([[True], work[1:] != work[:-1]]), np.arange(n), 0))]
    spell = (orig * 7 + 3) % n_spell
    odd = rng.random(n) < 0.02
    spell = np.where(odd, rng.integers(0, n_spell, n), spell)
    return [np.asarray(c, dtype=np.uint32) for c in (work, fan, orig, spell)]


@pytest.mark.parametrize("hash_bits", [None, "4"])
@pytest.mark.parametrize("n_works", [1, 65, 20_000])
@pytest.mark.parametrize("n_spell", [1, 50, 20_000])
def test_random_records(monkeypatch, n_spell, n_works, hash_bits):
    set_bits(monkeypatch, hash_bits)
    rng = np.random.default_rng(n_spell + 3 * n_works)
    cols = random_records(rng, 30_000, n_works, 3000, n_spell, rng.integers(0, 3000, 40))
    _, _, n = check(cols, n_works, 3000, n_spell, min_words=3)
    assert n > 300


@pytest.mark.parametrize("hash_bits", [None, "4"])
@pytest.mark.parametrize("n_script", [300, 1 << 19])
def test_200000_records(monkeypatch, n_script, hash_bits):
    set_bits(monkeypatch, hash_bits)
    rng = np.random.default_rng(n_script)
    cols = random_records(rng, 200_000, 5000, n_script, 997, rng.integers(0, n_script, 300))
    found, spans, n = check(cols, 5000, n_script, 997, min_words=4)
    assert n > 5000 and (found["n_passages"] > 5).sum() > 100 and (found["n_passages"] == 1).sum() > 1000
    check(cols, 5000, n_script, 997, min_words=4, max_gap=2)


# fs_readings.hip: k_rd_kept counts the kept runs of 256 runs, and the one-workgroup scan takes
# 1024 such counts per chunk
RUN_CHUNK = 1024 * 256


@pytest.mark.parametrize("n", [RUN_CHUNK - 1, RUN_CHUNK + 1])
def test_kept_runs_around_the_scan_s_chunk(monkeypatch, n):
    """Every record its own kept run (the fan index steps by 2): one run short of a chunk of
    the scan of the kept-run counts, and one run into its second chunk."""
    set_bits(monkeypatch, None)
    i = np.arange(n, dtype=np.int64)
    cols = [np.asarray(c, dtype=np.uint32) for c in (i * 7 // n, 2 * i, i * 7 % 40, i // 3 % 5)]
    found, spans, n_pass = check(cols, 7, 40, 5, min_words=1)
    assert n_pass == n and len(spans) == 40 and len(found) == 120
    assert int(found["n_passages"].sum()) == n


# ---- capacity and refusals -------------------------------------------------------------------

def call(cols, n_works, n_script, n_spell, min_words, max_gap, cap_r, cap_s, n_rows=None):
    L = _lib.load()
    found = np.zeros(max(cap_r, 1), dtype=abi.READING_DTYPE)
    spans = np.zeros(max(cap_s, 1), dtype=abi.READING_SPAN_DTYPE)
    got = [C.c_uint64(99) for _ in range(3)]
    rc = L.fs_readings(0, *(abi.ptr(c, C.c_uint32) for c in cols),
                       len(cols[0]) if n_rows is None else n_rows, n_works, n_script, n_spell,
                       min_words, max_gap, found.ctypes.data_as(C.c_void_p) if cap_r else None, cap_r,
                       spans.ctypes.data_as(C.c_void_p) if cap_s else None, cap_s,
                       *(C.byref(g) for g in got))
    return rc, [g.value for g in got], found, spans


def test_capacity_and_refusals():
    quotes = [(0, 9, line(1)), (1, 9, line(1)), (1, 9, line(2)), (2, 30, line(1)), (2, 9, line(1)[:5])]
    cols = layout(quotes)
    want_r, want_s, want_n = rr.readings(list(zip(*(c.tolist() for c in cols))), 3, 40, 1000, 5, 0)
    counts = [len(want_r), len(want_s), want_n]
    assert counts == [4, 3, 5]
    for cap_r, cap_s in ((0, 0), (3, 3), (4, 2), (3, 9), (4, 3), (9, 9)):
        rc, got, found, spans = call(cols, 3, 40, 1000, 5, 0, cap_r, cap_s)
        fits = cap_r >= 4 and cap_s >= 3
        assert rc == (abi.FS_OK if fits else abi.FS_E_CAPACITY) and got == counts
        if fits:
            assert [tuple(r) for r in found[:4].tolist()] == \
                [tuple(r[k] for k in rr.READING_KEYS) for r in want_r]
            assert [tuple(s) for s in spans[:3].tolist()] == \
                [tuple(s[k] for k in rr.SPAN_KEYS) for s in want_s]
        else:
            assert not found["n_words"].any() and not spans["n_passages"].any()
    ok = dict(n_works=3, n_script=40, n_spell=1000, min_words=5, max_gap=0, cap_r=9, cap_s=9)
    assert call(cols, **dict(ok, n_works=2))[0] == abi.FS_E_INVALID
    assert call(cols, **dict(ok, n_script=35))[0] == abi.FS_E_INVALID
    assert call(cols, **dict(ok, n_spell=int(cols[3].max()) + 1))[0] == abi.FS_OK
    assert call(cols, **dict(ok, n_spell=int(cols[3].max())))[0] == abi.FS_E_INVALID
    assert b"n_spell" in _lib.load().fs_last_error()
    assert call(cols, **dict(ok, min_words=0))[0] == abi.FS_E_INVALID
    swapped = [c.copy() for c in cols]
    for c in swapped:
        c[[3, 4]] = c[[4, 3]]
    assert call(swapped, **ok)[0] == abi.FS_E_INVALID
    assert b"sorted" in _lib.load().fs_last_error()
    back = [c[::-1].copy() for c in cols]
    assert call(back, **ok)[0] == abi.FS_E_INVALID
    assert call(cols, **dict(ok, n_script=(1 << 19) + 1))[0] == abi.FS_E_UNSUPPORTED
    assert call(cols, **ok, n_rows=1 << 32)[0] == abi.FS_E_UNSUPPORTED
    rc, got, _, _ = call(cols, **ok)
    assert rc == abi.FS_OK and got == counts
    ms = (C.c_double * 6)()
    assert _lib.load().fs_readings_times(ms) == abi.FS_OK and all(t > 0 for t in ms)


# ---- the command -----------------------------------------------------------------------------

def run_both(tmp_path, path, extra=(), tag="r"):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (tag, reader)))
        assert main(["readings", path, "-o", prefix, "--reader", reader, *extra]) == 0
        got[reader] = tuple(open(name, "rb").read() for name in readings.output_names(path, prefix))
    assert got["device"] == got["python"]
    return got["device"]


def options(min_words, max_gap, top, min_works, fold):
    return ["--min-words", str(min_words), "--max-gap", str(max_gap), "--top", str(top),
            "--min-works", str(min_works)] + (["--fold-case"] if fold else [])


@pytest.mark.parametrize("case,min_words,max_gap,top,min_works,fold", mrg.CASES)
def test_golden_cases_under_both_readers(tmp_path, bits, case, min_words, max_gap, top, min_works, fold):
    out = run_both(tmp_path, os.path.join(GOLDEN, mrg.INPUT),
                   options(min_words, max_gap, top, min_works, fold))
    for name, part in zip(mrg.golden_names(case), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_defaults_and_that_top_and_min_works_leave_the_spans_file_alone(tmp_path):
    path = os.path.join(GOLDEN, mrg.INPUT)
    base = run_both(tmp_path, path, tag="base")
    with open(os.path.join(GOLDEN, mrg.golden_names("default")[0]), "rb") as fh:
        assert base[0] == fh.read()
    cut = run_both(tmp_path, path, ["--top", "1", "--min-works", "2"], tag="cut")
    assert cut[1] == base[1] and len(cut[0]) < len(base[0])


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
    out = run_both(tmp_path, str(path), options(6, 0, 0, 1, False))
    assert b'fee""l""in' in out[0]
    assert out == tuple(p.encode("utf-8") for p in
                        rr.readings_csv(path.read_bytes().decode("utf-8"), 6, 0, 0, 1, False))


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
            main(["readings", str(path), "-o", str(tmp_path / "o"), "--reader", reader])
        errs.append(str(e.value.code))
    assert errs[0] == errs[1]
    assert errs[0].startswith("ao3.py readings: error: script word ") and "two scenes" in errs[0]


def test_after_a_search(tmp_path, monkeypatch, capsys):
    """The corpus of tests/test_gpu_cli_realistic.py and one more work that quotes a line in
    lower case."""
    from fandom_search_amd import search
    from tests import test_gpu_cli_realistic as real
    words, emb = real._table()
    np.savez(tmp_path / "vectors.npz", words=np.array(words), vectors=emb)
    monkeypatch.setenv("FANDOM_SEARCH_VECTORS", str(tmp_path / "vectors.npz"))
    search.set_vocab(None)
    (tmp_path / "script.txt").write_text(real.SCRIPT)
    fandir = tmp_path / "fan"
    fandir.mkdir()
    works = dict(real.FANWORKS)
    works["f.txt"] = "He said: i have a very bad feeling about this, Artoo! Never Tell Me the odds."
    for name, text in works.items():
        (fandir / name).write_text(text)
    monkeypatch.chdir(tmp_path)
    try:
        assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--window-size", "4"]) == 0
    finally:
        search.set_vocab(None)
    capsys.readouterr()
    dated = "match-4gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    text = open(dated, newline="", encoding="utf-8").read()
    want = rr.readings_csv(text, 4, 0, 0, 1, False)
    assert want[0].count("\r\n") > 2                       # readings beside the header
    out = run_both(tmp_path, dated, options(4, 0, 0, 1, False))
    assert out == tuple(p.encode("utf-8") for p in want)
    fold = run_both(tmp_path, dated, options(4, 1, 10, 1, True), tag="fold")
    assert fold == tuple(p.encode("utf-8") for p in rr.readings_csv(text, 4, 1, 10, 1, True))
