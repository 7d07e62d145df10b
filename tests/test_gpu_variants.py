"""`ao3.py variants` on the GPU: fs_matches_intern and fs_variants against their plain-Python
restatement (tests/variants_restated.py), equality throughout, and the command under both
readers against the committed expected CSVs."""

import csv
import ctypes as C
import datetime
import io
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, passages, variants
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests import variants_restated as vr
from tests.golden import make_variants_golden as mvg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 256 * 64             # bytes per workgroup of the reader's classifying kernels
FAN = 2                     # FAN_WORK_WORD
BITS = [None, "0", "4"]     # FS_INTERN_HASH_BITS: the default, every string collides, 16 hashes


def quoted(raw):
    return b'"' + raw.replace(b'"', b'""') + b'"'


def as_written(raw):
    """The field csv.writer would write for the bytes `raw`."""
    return quoted(raw) if any(c in raw for c in b',"\r\n') else raw


def file_of(fields, orig=None):
    """A match file whose FAN_WORK_WORD fields are `fields`, byte for byte as given."""
    return b"".join(b"w%d.txt,%d,%s,1,%d,s,2,ANNA,1,0.5,1,0.5\r\n"
                    % (k // 50, k, f, orig[k] if orig is not None else k % 7)
                    for k, f in enumerate(fields))


def set_bits(monkeypatch, bits):
    if bits is None:
        monkeypatch.delenv("FS_INTERN_HASH_BITS", raising=False)
    else:
        monkeypatch.setenv("FS_INTERN_HASH_BITS", bits)


def check_intern(tmp_path, fields, name="m.csv"):
    """fs_matches_intern over the file of `fields` against the restatement; returns the ids."""
    path = tmp_path / name
    path.write_bytes(file_of(fields))
    with MatchFile(str(path)) as mf:
        assert not mf.outside and mf.n == len(fields), mf.reason
        ids, first = mf.intern(FAN)
    want_ids, want_first = vr.intern(fields)
    assert ids.dtype == first.dtype == np.uint32
    assert ids.tolist() == want_ids and first.tolist() == want_first
    return ids


# ---- interning -----------------------------------------------------------------------------

@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_intern_sizes(tmp_path, monkeypatch, n, bits):
    set_bits(monkeypatch, bits)
    check_intern(tmp_path, [b"same"] * n)                     # every row on one slot
    check_intern(tmp_path, [b"f%d" % (n - k) for k in range(n)])         # all distinct
    rng = np.random.default_rng(n)
    check_intern(tmp_path, [b"v%d" % v for v in rng.integers(0, max(2, n // 3), n).tolist()])


def length_fields():
    out = []
    for length in (0, 1, 15, 16, 17, 63, 64, 65, 5000):
        base = bytes(97 + (k * 7 + length) % 26 for k in range(length))
        out += [base, base, base[:-1] + b"#" if length else b"#", base[:-1], base + b"z", base]
    return out + out[::-1]


@pytest.mark.parametrize("bits", BITS)
def test_intern_lengths_last_bytes_and_prefixes(tmp_path, monkeypatch, bits):
    set_bits(monkeypatch, bits)
    fields = length_fields()
    ids = check_intern(tmp_path, fields)
    assert len(set(ids.tolist())) == len(set(fields)) >= 30


@pytest.mark.parametrize("bits", BITS)
def test_intern_quoted_and_bare_and_non_ascii(tmp_path, monkeypatch, bits):
    set_bits(monkeypatch, bits)
    words = ["abc", "naïve", "中文", "\U0001f600", "a,b", 'say "hi"', "", "abc", "中文 "]
    fields = []
    for w in words:
        raw = w.encode("utf-8")
        fields += [as_written(raw), quoted(raw)]            # as csv.writer does, and quoted anyway
    path = tmp_path / "q.csv"
    path.write_bytes(file_of(fields))
    ids = check_intern(tmp_path, fields)
    assert ids[0] != ids[1] and ids[0] == ids[14]           # abc, "abc": two raw spellings
    with MatchFile(str(path)) as mf:
        raw_ids, first = mf.intern(FAN)
        texts = mf.text(FAN, first)
        remap, _, shown = variants.merge_spellings(texts)
    merged = np.take(remap, raw_ids).tolist()
    want = {}
    assert merged == [want.setdefault(w, len(want)) for w in words for _ in (0, 1)]
    assert shown == list(want)


@pytest.mark.parametrize("bits", BITS)
def test_intern_fields_across_a_tile_edge(tmp_path, monkeypatch, bits):
    """Padding rows in front of a few rows with long fields, the padding's length sweeping so
    that every byte of those fields comes to lie on either side of the reader's 16 KiB edge."""
    set_bits(monkeypatch, bits)
    pad = b"x" * 200
    k = (TILE - 700) // len(file_of([pad]))
    tail = [b"edge" * 20, b"edge" * 20 + b"!", quoted(b'ed"ge,' * 12), b"edge" * 20, b"",
            "né→中".encode("utf-8") * 9, quoted(b'ed"ge,' * 12)]
    crossed = set()
    for extra in range(0, 900, 7 if bits is None else 61):
        fields = [pad] * k + [b"y" * extra] + tail
        data = file_of(fields)
        crossed.add(len(data) > TILE > len(data) - len(file_of(tail)))
        check_intern(tmp_path, fields)
    assert crossed == {False, True}


@pytest.mark.parametrize("bits", [None, "4"])
def test_intern_200000_rows_20000_spellings(tmp_path, monkeypatch, bits):
    set_bits(monkeypatch, bits)
    rng = np.random.default_rng(7)
    ids = check_intern(tmp_path, [b"word%d" % v for v in rng.integers(0, 20000, 200_000).tolist()])
    assert 19_000 < int(ids.max()) + 1 <= 20_000


def test_intern_capacity_and_refusals(tmp_path):
    fields = [b"a", b"b", b"a", b"c", b"b"]
    path = tmp_path / "c.csv"
    path.write_bytes(file_of(fields))
    L = _lib.load()
    want_ids, want_first = vr.intern(fields)
    with MatchFile(str(path)) as mf:
        for cap in (0, 2, 3, 9):
            ids = np.full(5, 77, dtype=np.uint32)
            first = np.full(max(cap, 1), 77, dtype=np.uint32)
            got = C.c_uint64(99)
            rc = L.fs_matches_intern(mf._h, FAN, abi.ptr(ids, C.c_uint32),
                                     abi.ptr(first, C.c_uint32) if cap else None, cap, C.byref(got))
            assert rc == (abi.FS_OK if cap >= 3 else abi.FS_E_CAPACITY) and got.value == 3
            assert ids.tolist() == want_ids                  # complete either way
            assert first[:cap].tolist() == (want_first + [77] * cap)[:cap] if cap >= 3 else \
                (first == 77).all()
        got = C.c_uint64(99)
        assert L.fs_matches_intern(mf._h, 12, None, None, 0, C.byref(got)) == abi.FS_E_INVALID
    bad = tmp_path / "bad.csv"
    bad.write_bytes(file_of(fields) + b'x,1,"open')
    with MatchFile(str(bad)) as mf:
        assert mf.outside
        assert L.fs_matches_intern(mf._h, FAN, None, None, 0, C.byref(got)) == abi.FS_E_INVALID
    empty = tmp_path / "empty.csv"
    empty.write_bytes(b"")
    with MatchFile(str(empty)) as mf:
        ids, first = mf.intern(FAN)
        assert len(ids) == len(first) == 0


def test_intern_every_column_of_a_golden_input():
    path = os.path.join(GOLDEN, mvg.INPUT)
    rows = passages.read_matches(path)
    with MatchFile(path) as mf:
        for col in range(12):
            raw, first = mf.intern(col)
            remap, _, shown = variants.merge_spellings(mf.text(col, first))
            want = {}
            assert np.take(remap, raw).tolist() == [want.setdefault(r[col], len(want)) for r in rows]
            assert shown == list(want), col
            assert mf.intern_ms["device_total"] > 0


# ---- the group-by --------------------------------------------------------------------------

def check_variants(work, orig, spell, n_works, n_script, n_spell):
    """fs_variants against the restatement; returns (words, cells)."""
    words, cells = variants.find_variants(work, orig, spell, n_works, n_script, n_spell)
    recs = list(zip(np.asarray(work).tolist(), np.asarray(orig).tolist(), np.asarray(spell).tolist()))
    want_words, want_cells = vr.variants(recs, n_works, n_script, n_spell)
    assert [tuple(c) for c in cells.tolist()] == [tuple(c[k] for k in vr.CELL_KEYS) for c in want_cells]
    have = [o for o, w in enumerate(want_words) if w["n_records"]]
    assert np.flatnonzero(words["n_records"]).tolist() == have
    assert [tuple(w) for w in words[have].tolist()] == \
        [tuple(want_words[o][k] for k in vr.WORD_KEYS) for o in have]
    rest = np.delete(words, have)
    assert (rest["first_cell"] == vr.NONE).all()
    assert not any(rest[k].any() for k in vr.WORD_KEYS[:-1])
    return words, cells


def test_zero_and_one_record():
    words, cells = variants.find_variants([], [], [], 0, 3, 0)
    assert len(cells) == 0 and (words["first_cell"] == vr.NONE).all() and not words["n_records"].any()
    words, cells = check_variants([4], [2], [6], 5, 3, 7)
    assert cells.tolist() == [(2, 6, 1, 1)] and words[2].tolist() == (1, 1, 1, 0)


@pytest.mark.parametrize("n_works", [1, 65, 100_000])
@pytest.mark.parametrize("n_spell", [1, 50, 100_000])
@pytest.mark.parametrize("n_script", [1, 300, 1 << 19])
def test_random_records(n_script, n_spell, n_works):
    rng = np.random.default_rng(n_script + 3 * n_spell + 7 * n_works)
    n = 50_000
    # a skewed choice of script words and spellings: cells of one record and of thousands
    orig = (rng.random(n) ** 3 * n_script).astype(np.uint32)
    spell = ((rng.random(n) ** 2 * n_spell).astype(np.uint32) + orig) % n_spell
    work = rng.integers(0, n_works, n).astype(np.uint32)
    check_variants(work, orig, spell, n_works, n_script, n_spell)


def test_shuffled_records_give_the_output_of_sorted_ones():
    rng = np.random.default_rng(3)
    n = 20_000
    work, orig, spell = (rng.integers(0, m, n).astype(np.uint32) for m in (40, 200, 30))
    order = np.lexsort((spell, orig, work))
    a = variants.find_variants(work[order], orig[order], spell[order], 40, 200, 30)
    for perm in (np.arange(n), rng.permutation(n), order[::-1]):
        b = variants.find_variants(work[perm], orig[perm], spell[perm], 40, 200, 30)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    check_variants(work, orig, spell, 40, 200, 30)


@pytest.mark.parametrize("n_spell", [1, 64, 65, 1000])
def test_one_word_of_many_spellings(n_spell):
    """64 cells are ranked by a lane each, 65 by the wave; short words sit in the same waves."""
    rng = np.random.default_rng(n_spell)
    spell = np.concatenate([np.arange(n_spell), rng.integers(0, n_spell, 3 * n_spell)]).astype(np.uint32)
    orig = np.full(len(spell), 5, dtype=np.uint32)
    work = rng.integers(0, 9, len(spell)).astype(np.uint32)
    few = np.arange(12, dtype=np.uint32)
    words, cells = check_variants(np.concatenate([few % 2, work]), np.concatenate([few % 4 + 6, orig]),
                                  np.concatenate([few % 3 % n_spell, spell]), 9, 10, n_spell)
    assert int(words[5]["n_spellings"]) == n_spell


def test_all_records_on_one_cell_and_ties():
    n = 30_000
    words, cells = check_variants(np.arange(n) % 7, np.full(n, 2), np.full(n, 3), 7, 4, 5)
    assert cells.tolist() == [(2, 3, n, 7)]
    # ties in n_records that n_works breaks, and ties in both that the spelling id breaks
    work = [0, 0, 0, 1, 0, 1, 0, 0, 1, 1]
    spell = [3, 3, 2, 2, 1, 1, 0, 4, 4, 4]
    _, cells = check_variants(work, [1] * 10, spell, 2, 2, 5)
    assert [c[1] for c in cells.tolist()] == [4, 1, 2, 3, 0]


def test_refusals_and_capacity():
    L = _lib.load()
    work, orig, spell = (abi.as_u32(v) for v in ([0, 1, 1, 0], [2, 2, 3, 0], [1, 0, 1, 1]))
    want_words, want_cells = vr.variants(list(zip(work.tolist(), orig.tolist(), spell.tolist())), 2, 4, 2)

    def call(cap, n_works=2, n_script=4, n_spell=2):
        words = np.zeros(n_script, dtype=abi.VARIANT_WORD_DTYPE)
        cells = np.zeros(max(cap, 1), dtype=abi.VARIANT_CELL_DTYPE)
        got = C.c_uint64(99)
        rc = L.fs_variants(0, abi.ptr(work, C.c_uint32), abi.ptr(orig, C.c_uint32),
                           abi.ptr(spell, C.c_uint32), 4, n_works, n_script, n_spell,
                           words.ctypes.data_as(C.c_void_p),
                           cells.ctypes.data_as(C.c_void_p) if cap else None, cap, C.byref(got))
        return rc, got.value, words, cells
    for cap in (0, 3, 4):
        rc, got, words, cells = call(cap)
        assert rc == (abi.FS_OK if cap == 4 else abi.FS_E_CAPACITY) and got == 4
        assert [tuple(w) for w in words.tolist()] == \
            [tuple(w[k] for k in vr.WORD_KEYS) for w in want_words]      # complete either way
        if cap == 4:
            assert [tuple(c) for c in cells.tolist()] == \
                [tuple(c[k] for k in vr.CELL_KEYS) for c in want_cells]
    assert call(4, n_works=1)[0] == abi.FS_E_INVALID
    assert call(4, n_script=3)[0] == abi.FS_E_INVALID
    assert call(4, n_spell=1)[0] == abi.FS_E_INVALID
    assert b"n_spell" in L.fs_last_error()
    got = C.c_uint64(0)
    assert L.fs_variants(0, None, None, None, 4, 2, (1 << 19) + 1, 2, None, None, 0,
                         C.byref(got)) == abi.FS_E_INVALID     # (no words buffer)
    words = np.zeros((1 << 19) + 1, dtype=abi.VARIANT_WORD_DTYPE)
    assert L.fs_variants(0, abi.ptr(work, C.c_uint32), abi.ptr(orig, C.c_uint32),
                         abi.ptr(spell, C.c_uint32), 4, 2, (1 << 19) + 1, 2,
                         words.ctypes.data_as(C.c_void_p), None, 0,
                         C.byref(got)) == abi.FS_E_UNSUPPORTED


# ---- the command ---------------------------------------------------------------------------

def run_both(tmp_path, path, extra=(), tag="v"):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (tag, reader)))
        assert main(["variants", path, "-o", prefix, "--reader", reader, *extra]) == 0
        got[reader] = tuple(open(name, "rb").read() for name in variants.output_names(path, prefix))
    assert got["device"] == got["python"]
    return got["device"]


def options(top, min_records, fold):
    return ["--top", str(top), "--min-records", str(min_records)] + (["--fold-case"] if fold else [])


@pytest.mark.parametrize("case,top,min_records,fold", mvg.CASES)
def test_golden_cases_under_both_readers(tmp_path, case, top, min_records, fold):
    out = run_both(tmp_path, os.path.join(GOLDEN, mvg.INPUT), options(top, min_records, fold))
    for name, part in zip(mvg.golden_names(case), out):
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert part == fh.read(), name


def test_defaults_and_that_top_and_min_records_leave_the_words_file_alone(tmp_path):
    path = os.path.join(GOLDEN, mvg.INPUT)
    base = run_both(tmp_path, path, tag="base")
    with open(os.path.join(GOLDEN, mvg.golden_names("default")[0]), "rb") as fh:
        assert base[0] == fh.read()
    cut = run_both(tmp_path, path, options(1, 3, False), tag="cut")
    assert cut[1] == base[1] and len(cut[0]) < len(base[0])


def run_command(argv):
    try:
        main(argv)
        return None
    except (Exception, SystemExit) as e:
        return type(e), str(e)


def test_an_off_grammar_file_gives_the_python_reader_s_output(tmp_path):
    with open(os.path.join(GOLDEN, mvg.INPUT), "rb") as fh:
        lines = fh.read().split(b"\r\n")
    parts = lines[5].split(b",")
    parts[2] = b'fee"l"in'                       # a quote inside a field: csv.reader takes it
    lines[5] = b",".join(parts)
    path = tmp_path / "m.csv"
    path.write_bytes(b"\r\n".join(lines))
    with MatchFile(str(path)) as mf:
        assert mf.outside and mf.reason & abi.FS_MATCH_BAD_OPEN
    out = run_both(tmp_path, str(path), options(0, 1, False))
    assert b'"fee""l""in"' in out[0]
    assert out == tuple(p.encode("utf-8") for p in
                        vr.variants_csv(path.read_bytes().decode("utf-8"), 0, 1, False))


def test_two_labels_for_one_script_word(tmp_path):
    with open(os.path.join(GOLDEN, mvg.INPUT), newline="", encoding="utf-8") as fh:
        rows = list(csv.reader(fh))
    rows[40][8] = "99"                            # the same script word in another scene
    buf = io.StringIO(newline="")
    csv.writer(buf).writerows(rows)
    path = tmp_path / "m.csv"
    path.write_bytes(buf.getvalue().encode("utf-8"))
    errs = [run_command(["variants", str(path), "-o", str(tmp_path / "o"), "--reader", r])
            for r in ("device", "python")]
    assert errs[0] == errs[1] and errs[0][0] is SystemExit
    assert errs[0][1].startswith("ao3.py variants: error: script word ") and "two scenes" in errs[0][1]


def test_the_device_path_decodes_no_per_record_text(tmp_path, monkeypatch):
    n = 100_000
    rng = np.random.default_rng(5)
    orig = rng.integers(0, 400, n)
    fan = (orig * 31 + rng.integers(0, 3, n) ** 2) % 997
    path = tmp_path / "big.csv"
    with open(path, "w", newline="", encoding="utf-8") as fh:
        csv.writer(fh).writerows(
            ("w%05d.txt" % (k // 100), k, "f%d" % f, 1, o, "s%d" % o, 2, "ANNA", o // 50, 0.25, 3, 0.5)
            for k, (o, f) in enumerate(zip(orig.tolist(), fan.tolist())))
    asked = []
    text = MatchFile.text

    def counting(self, column, records):
        asked.append((column, len(records)))
        return text(self, column, records)
    monkeypatch.setattr(MatchFile, "text", counting)
    prefix = str(tmp_path / "dev")
    assert main(["variants", str(path), "-o", prefix, "--reader", "device"]) == 0
    monkeypatch.setattr(MatchFile, "text", text)
    n_distinct = len(set(fan.tolist()))
    words_with_a_record = len(set(orig.tolist()))
    heads, deferred = n // 100, 0                 # (0.25 and 0.5: nothing is left to the host)
    assert n_distinct < 1000
    assert sum(k for _, k in asked) <= n_distinct + 3 * words_with_a_record + heads + deferred
    assert (FAN, n_distinct) in asked
    want = vr.variants_csv(path.read_bytes().decode("utf-8"))
    assert tuple(open(p, newline="", encoding="utf-8").read()
                 for p in variants.output_names(str(path), prefix)) == want


def test_after_a_search(tmp_path, monkeypatch, capsys):
    """The corpus of tests/test_gpu_cli_realistic.py (capitalised tokens, synonym swaps, names
    outside the vocabulary) and one more work that quotes a line in lower case."""
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
    want = vr.variants_csv(open(dated, newline="", encoding="utf-8").read(), top=0)
    cells = list(csv.reader(io.StringIO(want[0])))[1:]
    words_rows = list(csv.reader(io.StringIO(want[1])))[1:]
    assert any(int(r[6]) >= 2 for r in words_rows)        # a script word with two spellings
    assert any(r[8] == "0" for r in cells)                # a fan word that is not the script's
    out = run_both(tmp_path, dated, options(0, 1, False))
    assert out == tuple(p.encode("utf-8") for p in want)
    run_both(tmp_path, dated, options(10, 1, True), tag="fold")
