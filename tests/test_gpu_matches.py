"""The match CSV read on the GPU (fs_matches_*, fandom_search_amd/matches.py) against the Python
reader it replaces: passages.read_matches + sort_records are the oracle for rows, field texts,
numbers (as bit patterns), work ids, order and names; `passages`, `works` and `quotes` must
write the same bytes, or raise the same error, under --reader device and --reader python."""

import csv
import datetime
import io
import os

import numpy as np
import pytest

from fandom_search_amd import abi, passages, synth
from fandom_search_amd.cli import main
from fandom_search_amd.matches import MatchFile
from tests.golden import make_passages_golden as mpg

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIELDS = passages.FIELDS
TILE = 256 * 64             # bytes per workgroup of the classifying kernels
WRITER_FILES = []           # (name, status, n_rows, n_deferred) of every file the writer made


def row(name, fan, orig, word="w", oword="s", char="ANNA", scene=1, dist=0.25, lev=1, comb=0.25):
    return [name, fan, word, 11, orig, oword, 22, char, scene, dist, lev, comb]


def csv_bytes(rows, header=False, terminator="\r\n"):
    buf = io.StringIO()
    w = csv.writer(buf, lineterminator=terminator)
    if header:
        w.writerow(FIELDS)
    w.writerows(rows)
    return buf.getvalue().encode("utf-8")


def some_rows(n=40, seed=0):
    rng = np.random.default_rng(seed)
    out, fan = [], 0
    for k in range(n):
        fan += int(rng.integers(0, 3))
        o = 100 + k
        out.append(row("work%d.txt" % (k // 9), fan, o, "f%d" % k, "s%d" % o, "C%d" % (o % 3),
                       o // 7, float(rng.random()) * 0.1, int(rng.integers(0, 5)),
                       float(rng.random())))
    return out


def check_parity(path, writer_made=True):
    """MatchFile(path) against read_matches + sort_records; returns the MatchFile."""
    rows = passages.read_matches(path)
    want = passages.sort_records(rows)
    mf = MatchFile(path)
    assert not mf.outside, (path, mf.reason)
    if writer_made:
        WRITER_FILES.append((os.path.basename(str(path)), mf.status, mf.n, mf.n_deferred))
        assert mf.n_deferred * 1000 <= mf.n, (mf.n_deferred, mf.n)
    assert mf.n == len(rows)
    with open(path, newline="", encoding="utf-8") as fh:
        first = next((r for r in csv.reader(fh) if r), None)
    assert mf.has_header == (first == FIELDS)
    got = mf.sorted()
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        if a.dtype.kind == "f":
            a, b = a.view(np.uint64), b.view(np.uint64)
        assert np.array_equal(a, b)
    assert mf.names == list(dict.fromkeys(r[0] for r in rows))
    assert np.array_equal(mf.lev, np.array([int(r[10]) for r in rows], dtype=np.uint32))
    everyone = np.arange(len(rows))
    for col in range(12):
        assert mf.text(col, everyone) == [r[col] for r in rows], col
    for col in (9, 11):
        vals = (mf.dist if col == 9 else mf.comb).view(np.uint64)
        ref = np.array([passages._distance(r[col]) for r in rows], dtype=np.float64).view(np.uint64)
        assert np.array_equal(vals, ref)
    return mf


def write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


# ---- parity ------------------------------------------------------------------------------

@pytest.mark.parametrize("src", sorted(set(c[1] for c in mpg.CASES)))
def test_golden_inputs_with_and_without_header(tmp_path, src):
    path = os.path.join(GOLDEN, src)
    check_parity(path)
    rows = passages.read_matches(path)
    with open(path, newline="", encoding="utf-8") as fh:
        had = next(csv.reader(fh)) == FIELDS
    check_parity(write(tmp_path, "other.csv", csv_bytes(rows, header=not had)))


def odd_rows():
    rows = some_rows(30, seed=3)
    rows[1][2] = "a,b"
    rows[2][2] = 'say "hi"'
    rows[3][5] = "line\r\nbreak"
    rows[4][5] = "lone\nnewline"
    rows[5][2] = '"'
    rows[6][2] = '""",'
    rows[7][2] = "naïve 中文 \U0001f600"
    rows[8][7] = "ÉLISE"
    rows[9][9] = ""
    rows[10][11] = ""
    rows[11][9] = float("nan")
    rows[12][9] = float("inf")
    rows[13][11] = float("-inf")
    rows[14][9] = -0.0
    rows[15][9] = 5e-324
    rows[16][9] = 1.7976931348623157e308
    rows[17][2] = " "
    rows[18][2] = "\n"
    rows[19][0] = "dir,with comma/w.txt"
    rows[20][0] = "dir,with comma/w.txt"
    return rows


@pytest.mark.parametrize("header", [False, True])
@pytest.mark.parametrize("terminator", ["\r\n", "\n"])
def test_odd_fields(tmp_path, header, terminator):
    check_parity(write(tmp_path, "odd.csv", csv_bytes(odd_rows(), header, terminator)))


def test_blank_lines_and_a_last_row_without_terminator(tmp_path):
    data = csv_bytes(some_rows(12, seed=5))
    lines = data.split(b"\r\n")
    blank = b"\r\n".join([b"", lines[0], b"", b"", *lines[1:6], b""] + lines[6:-1])
    mf = check_parity(write(tmp_path, "blank.csv", b"\r\n\n" + blank + b"\n\r\n"), False)
    assert mf.n == 12
    check_parity(write(tmp_path, "noterm.csv", data[:-2]), False)
    check_parity(write(tmp_path, "noterm_lf.csv", csv_bytes(some_rows(3), True, "\n")[:-1]), False)


def test_one_row_header_only_and_empty(tmp_path):
    assert check_parity(write(tmp_path, "one.csv", csv_bytes(some_rows(1)))).n == 1
    assert check_parity(write(tmp_path, "one_h.csv", csv_bytes(some_rows(1), True))).n == 1
    for name, data in (("h.csv", csv_bytes([], True)), ("h_lf.csv", csv_bytes([], True, "\n")),
                       ("h_bare.csv", csv_bytes([], True)[:-2]), ("empty.csv", b""),
                       ("blank.csv", b"\r\n\r\n")):
        mf = check_parity(write(tmp_path, name, data), False)
        assert mf.n == 0 and mf.names == [] and mf.has_header == name.startswith("h")


def test_works_that_come_back_and_records_out_of_order(tmp_path):
    rows = some_rows(60, seed=7)
    for k in (20, 21, 22, 50):
        rows[k][0] = "work0.txt"              # comes back later in the file
    rows[30][1], rows[33][1] = rows[33][1] + 5, 0
    rng = np.random.default_rng(1)
    mixed = [rows[k] for k in rng.permutation(len(rows))]
    for name, rr in (("back.csv", rows), ("mixed.csv", mixed)):
        mf = check_parity(write(tmp_path, name, csv_bytes(rr)))
        assert not np.array_equal(mf.order(), np.arange(mf.n))


def test_a_name_quoted_in_one_row_and_not_in_the_next(tmp_path):
    data = csv_bytes(some_rows(9, seed=9))           # one work
    lines = data.split(b"\r\n")
    lines[3] = b'"work0.txt"' + lines[3][len(b"work0.txt"):]
    lines[4] = b'"work0.txt"' + lines[4][len(b"work0.txt"):]
    mf = check_parity(write(tmp_path, "q.csv", b"\r\n".join(lines)), False)
    assert mf.names == ["work0.txt"] and int(mf.ix["head"].sum()) == 3


def test_fields_float_reads_but_the_kernel_leaves_alone(tmp_path):
    data = csv_bytes(some_rows(9, seed=11))
    lines = data.split(b"\r\n")
    for k, text in ((1, b"+0.5"), (2, b"1_0.5"), (3, b" 0.25"), (4, b"Infinity"),
                    (5, b"0.1234567890123456789")):
        lines[k] = lines[k].rsplit(b",", 1)[0] + b"," + text
    mf = check_parity(write(tmp_path, "defer.csv", b"\r\n".join(lines)), False)
    assert mf.status == abi.FS_MATCHES_DEFERRED and mf.n_deferred == 5


@pytest.mark.parametrize("stage", ["0", "1"])
def test_tile_edges(tmp_path, monkeypatch, stage):
    """Padding rows in front of a small set of rows, the padding's length sweeping over two
    tiles: every terminator, "" pair and quoted newline lands on every position around a tile
    edge (and around every lane's 64 bytes on the way)."""
    monkeypatch.setenv("FS_MATCHES_STAGE", stage)
    tail = csv_bytes(odd_rows()[:8])
    pad_row = csv_bytes([row("pad.txt", 1, 2, "x" * 200)])
    bare = len(csv_bytes([row("pad.txt", 1, 2, "")]))

    def padded(off):                               # the tail's first byte at offset `off`
        k = (off - bare) // len(pad_row)
        return pad_row * k + csv_bytes([row("pad.txt", 1, 2, "y" * (off - bare - k * len(pad_row)))])

    reach = len(tail) + 8                          # the whole tail passes over the edge
    offsets = list(range(TILE - reach, TILE + 9)) + list(range(2 * TILE - reach, 2 * TILE + 9, 5)) + \
        list(range(1000, 2 * TILE, 509))
    for off in (offsets if stage == "1" else offsets[::9]):
        data = padded(off) + tail
        assert data[off:] == tail
        check_parity(write(tmp_path, "edge.csv", data))


# ---- off-grammar files -------------------------------------------------------------------

def off_grammar_files():
    good = csv_bytes(some_rows(6, seed=13))
    lines = good.split(b"\r\n")

    def with_line(k, new):
        return b"\r\n".join(lines[:k] + [new] + lines[k + 1:])

    def field(k, col, text):
        parts = lines[k].split(b",")
        parts[col] = text
        return with_line(k, b",".join(parts))
    return [
        ("quote_inside_field", abi.FS_MATCH_BAD_OPEN, field(2, 2, b'ab"c"')),
        ("text_behind_closing_quote", abi.FS_MATCH_BAD_CLOSE, field(2, 2, b'"ab"c')),
        ("file_ends_in_quotes", abi.FS_MATCH_BAD_CLOSE, good + b'x,1,"open'),
        ("lone_cr", abi.FS_MATCH_BAD_CR, field(3, 2, b"a\rb")),
        ("nul", abi.FS_MATCH_BAD_NUL, field(3, 2, b"a\x00b")),
        ("eleven_fields", abi.FS_MATCH_BAD_FIELDS, with_line(1, lines[1].rsplit(b",", 1)[0])),
        ("thirteen_fields", abi.FS_MATCH_BAD_FIELDS, with_line(1, lines[1] + b",9")),
        ("signed_index", abi.FS_MATCH_BAD_INT, field(1, 1, b"+5")),
        ("negative_index", abi.FS_MATCH_BAD_INT, field(1, 4, b"-5")),
        ("spaced_index", abi.FS_MATCH_BAD_INT, field(1, 1, b" 5")),
        ("underscore_index", abi.FS_MATCH_BAD_INT, field(1, 1, b"1_0")),
        ("quoted_index", abi.FS_MATCH_BAD_INT, field(1, 4, b'"5"')),
        ("index_of_2_32", abi.FS_MATCH_BAD_INT, field(1, 1, b"4294967296")),
        ("eleven_digits", abi.FS_MATCH_BAD_INT, field(1, 1, b"00000000005")),
        ("empty_lev", abi.FS_MATCH_BAD_INT, field(1, 10, b"")),
        ("bad_utf8", abi.FS_MATCH_BAD_UTF8, field(2, 2, b"a\xffb")),
        ("cut_utf8", abi.FS_MATCH_BAD_UTF8, field(2, 2, b"a\xe4\xb8")),
        ("overlong_utf8", abi.FS_MATCH_BAD_UTF8, field(2, 2, b"\xc0\xaf")),
        ("surrogate_utf8", abi.FS_MATCH_BAD_UTF8, field(2, 2, b"\xed\xa0\x80")),
        ("quoted_header", 0, b'"FAN_WORK_FILENAME",' + csv_bytes([], True)[18:] + good),
        ("distance_float_refuses", None, field(2, 9, b"abc")),
    ]


def run_command(argv):
    try:
        main(argv)
        return None
    except (Exception, SystemExit) as e:          # SystemExit: cli's "ao3.py works: error: ..."
        return type(e), str(e)


@pytest.mark.parametrize("name,reason,data", off_grammar_files(), ids=lambda v: v if isinstance(v, str) else "")
def test_off_grammar_files(tmp_path, name, reason, data):
    path = write(tmp_path, "m.csv", data)
    mf = MatchFile(path)
    assert mf.outside
    if reason:
        assert mf.status == abi.FS_MATCHES_OUTSIDE and mf.reason & reason, (mf.reason, reason)
    for cmd in ("passages", "works", "quotes"):
        outs = {}
        for reader in ("device", "python"):
            prefix = str(tmp_path / ("%s_%s" % (cmd, reader)))
            err = run_command([cmd, path, "-o", prefix, "--min-words", "2", "--reader", reader])
            files = sorted(f for f in os.listdir(tmp_path) if f.startswith("%s_%s" % (cmd, reader)))
            outs[reader] = (err, [(f[len(cmd) + len(reader) + 1:], (tmp_path / f).read_bytes())
                                  for f in files])
        assert outs["device"] == outs["python"], cmd


def test_two_labels_for_one_script_word(tmp_path):
    rows = some_rows(20, seed=17)
    rows[12][4], rows[12][5] = rows[3][4], rows[3][5]       # same word, another scene
    rows[12][7], rows[12][8] = rows[3][7], 99
    path = write(tmp_path, "m.csv", csv_bytes(rows))
    with MatchFile(path) as mf:
        assert not mf.outside and mf.labels(8, int(mf.orig.max()) + 1) is None
        assert mf.label_rows(8, int(mf.orig.max()) + 1)[1] == 1
    for cmd in ("works", "quotes"):
        errs = [run_command([cmd, path, "-o", str(tmp_path / "o"), "--reader", r])
                for r in ("device", "python")]
        assert errs[0] == errs[1] and errs[0] is not None and "two scenes" in errs[0][1]


# ---- the commands --------------------------------------------------------------------------

def both_readers(tmp_path, cmd, path, extra=()):
    got = {}
    for reader in ("device", "python"):
        prefix = str(tmp_path / ("%s_%s" % (cmd, reader)))
        assert main([cmd, path, "-o", prefix, "--reader", reader, *extra]) == 0
        files = sorted(f for f in os.listdir(tmp_path) if f.startswith("%s_%s" % (cmd, reader)))
        assert files
        got[reader] = [(f[len(cmd) + len(reader) + 1:], (tmp_path / f).read_bytes()) for f in files]
    assert got["device"] == got["python"]
    return got["device"]


@pytest.mark.parametrize("case,src,m,g", mpg.CASES)
def test_commands_on_golden_inputs(tmp_path, case, src, m, g):
    path = os.path.join(GOLDEN, src)
    args = ("--min-words", str(m), "--max-gap", str(g))
    out = both_readers(tmp_path, "passages", path, args)
    with open(os.path.join(GOLDEN, mpg.golden_name(case, m, g)), "rb") as fh:
        assert out[0][1] == fh.read()
    both_readers(tmp_path, "works", path, args)
    both_readers(tmp_path, "quotes", path, args)
    both_readers(tmp_path, "quotes", path, args + ("--min-works", "2"))


def test_commands_on_odd_fields(tmp_path):
    rows = odd_rows()
    for k, r in enumerate(rows):               # runs long enough to make passages
        r[0], r[1], r[4], r[7], r[8] = "w%d" % (k // 10), k, 500 + k, "A,\"B\"", "1\n2"
    path = write(tmp_path, "odd.csv", csv_bytes(rows, True))
    for cmd in ("passages", "works", "quotes"):
        both_readers(tmp_path, cmd, path, ("--min-words", "3"))


def test_commands_after_a_search(tmp_path, monkeypatch, synth_base):
    from fandom_search_amd import search
    words = synth_base["words"]
    script = synth.script_tokens(3000)
    fandir = tmp_path / "fanworks"
    synth.write_corpus(str(fandir), 40, 1500, script, words)
    (tmp_path / "script.txt").write_text(synth.script_markup(script, words))
    monkeypatch.chdir(tmp_path)
    search.set_vocab(None)
    monkeypatch.delenv("FANDOM_SEARCH_VECTORS", raising=False)
    assert main(["search", str(fandir), str(tmp_path / "script.txt"), "--synthetic-vocab"]) == 0
    dated = "match-6gram-%s.csv" % '{:%Y%m%d}'.format(datetime.date.today())
    mf = check_parity(dated)
    assert mf.n > 1000 and mf.has_header and mf.status == abi.FS_MATCHES_PARSED
    out = tmp_path / "out"
    out.mkdir()
    for cmd in ("passages", "works", "quotes"):
        assert len(both_readers(out, cmd, dated)[0][1]) > 200


# ---- scale ---------------------------------------------------------------------------------

def big_file(path, n, seed=1):
    """n records in passages_bench's mix, written through csv.writer; returns the columns."""
    rng = np.random.default_rng(seed)
    work = np.cumsum(rng.random(n) < 1e-3)
    fstep = rng.choice([0, 1, 2], size=n, p=[0.02, 0.9, 0.08])
    fan = np.cumsum(fstep)
    ostep = np.where(rng.random(n) < 0.9, fstep, rng.integers(-40, 40, size=n))
    orig = np.cumsum(ostep) + 40 * n + 1
    dist = rng.random(n) * 0.1
    comb = dist * rng.integers(0, 8, size=n)
    with open(path, "w", newline="", encoding="utf-8") as fh:
        w = csv.writer(fh)
        w.writerows(zip(("w%07d.txt" % k for k in work.tolist()), fan.tolist(),
                        ("f%d" % (o % 997) for o in orig.tolist()), (1 for _ in range(n)),
                        orig.tolist(), ("s%d" % (o % 991) for o in orig.tolist()),
                        (2 for _ in range(n)), ("ANNA" for _ in range(n)), (1 for _ in range(n)),
                        dist.tolist(), (3 for _ in range(n)), comb.tolist()))
    return work, fan, orig, dist, comb


def test_ten_million_records(tmp_path):
    """Against numpy's own parse of the columns, not the Python reader."""
    path = str(tmp_path / "big.csv")
    n = 10_000_000
    big_file(path, n)
    ref = np.loadtxt(path, delimiter=",", usecols=(1, 4, 9, 10, 11), dtype=np.float64)
    names = np.loadtxt(path, delimiter=",", usecols=(0,), dtype="U12")
    with MatchFile(path) as mf:
        WRITER_FILES.append(("big.csv", mf.status, mf.n, mf.n_deferred))
        assert not mf.outside and mf.n == n and mf.n_deferred == 0
        assert np.array_equal(mf.fan, ref[:, 0].astype(np.uint32))
        assert np.array_equal(mf.orig, ref[:, 1].astype(np.uint32))
        assert np.array_equal(mf.lev, ref[:, 3].astype(np.uint32))
        assert np.array_equal(mf.dist.view(np.uint64), ref[:, 2].copy().view(np.uint64))
        assert np.array_equal(mf.comb.view(np.uint64), ref[:, 4].copy().view(np.uint64))
        uniq, first, inv = np.unique(names, return_index=True, return_inverse=True)
        assert mf.names == uniq[np.argsort(first)].tolist()          # (the names ascend)
        assert np.array_equal(mf.work, np.argsort(np.argsort(first))[inv])
        assert np.array_equal(mf.order(), np.arange(n))
        pick = np.random.default_rng(2).integers(0, n, 1000)
        assert mf.text(0, pick) == names[pick].tolist()


def test_passages_of_a_million_records_under_both_readers(tmp_path):
    path = str(tmp_path / "m.csv")
    big_file(path, 1_000_000, seed=4)
    assert both_readers(tmp_path, "passages", path)[0][1].count(b"\r\n") > 1000


def test_the_writer_s_files_were_never_outside():
    """Runs last: every file of this module that csv.writer produced was parsed, with at most
    one numeric field per 1000 rows left to the host (each check_parity asserted it)."""
    assert len(WRITER_FILES) > 20
    for name, status, n, deferred in WRITER_FILES:
        assert status != abi.FS_MATCHES_OUTSIDE and deferred * 1000 <= n, (name, status, n, deferred)
