"""The device match reader (fs_matches_*, fandom_search_amd/matches.py) away from the middle of
a file and off the narrow numbers tests/test_gpu_matches.py writes: doubles of every exponent,
ties and subnormals through the kernel's own fs_dec instantiation; every refusal planted on
both sides of a lane (64 B), wave (4096 B) and tile (16384 B) edge, at the file's first bytes
and at its last; the quoting parity carried over the scan's 1024-tile chunk; both sides of the
deferred list's bound and of the LDS stage's size switch; and single-byte mutants of a good
file.  The oracle is tests/matches_restated.py (pinned to csv.reader and bytes.decode by
tests/test_matches_restated_host.py) for what is outside and why, and the Python reader
(check_parity of tests/test_gpu_matches.py) or float() for what is inside.  Every comparison is
equality of bits or bytes; every test runs under FS_MATCHES_STAGE 0 and 1."""

import functools

import numpy as np
import pytest

from fandom_search_amd import abi, passages
from fandom_search_amd.matches import MatchFile
from tests import matches_restated as mr
from tests.test_gpu_matches import both_readers, check_parity, csv_bytes, row, write

pytestmark = pytest.mark.gpu

LANE, WAVE, TILE = 64, 4096, 16384
EDGES = (LANE, WAVE, TILE, 2 * TILE)


@pytest.fixture(params=["0", "1"])
def stage(request, monkeypatch):
    monkeypatch.setenv("FS_MATCHES_STAGE", request.param)
    return request.param


# ---- rows of a chosen length, written without csv.writer ----------------------------------

def plain_row(fan, orig, word=b"w", dist=b"0.5", comb=b"0.25", name=b"p.txt"):
    return b"%s,%d,%s,11,%d,s,22,ANNA,1,%s,3,%s\r\n" % (name, fan, word, orig, dist, comb)


TINY = len(b"p,7,,1,8,s,2,A,1,,3,\r\n")


def sized_row(length):
    """A valid row of exactly `length` bytes (its terminator counted), length >= TINY."""
    assert length >= TINY, length
    return b"p,7,%s,1,8,s,2,A,1,,3,\r\n" % (b"x" * (length - TINY))


def padding(total):
    """Valid rows of `total` bytes together: 0, or TINY and more."""
    if total == 0:
        return b""
    k = (total - TINY) // 240
    return sized_row(240) * k + sized_row(total - 240 * k)


def assert_verdict(tmp_path, data, what=""):
    """MatchFile of `data` against the restatement: outside or not, the reason when outside,
    the Python reader's every row, field and number when not.  Returns the MatchFile."""
    path = write(tmp_path, "m.csv", data)
    v = mr.verdict(data)
    mf = MatchFile(path)
    assert (mf.status == abi.FS_MATCHES_OUTSIDE) == v[0], (what, mf.status, mf.reason, v)
    if v[0]:
        assert mf.outside and mf.reason == v[1], (what, mf.reason, v)
        return mf
    assert (mf.status, mf.has_header, mf.n, mf.n_deferred) == (mr.status_of(v), v[2], v[3], v[4]), \
        (what, mf.status, mf.n, mf.n_deferred, v)
    if mf.outside:
        # parsed on the device; float() refused a deferred field on the host, and the Python
        # reader says so as it always did
        refused = 0
        records = mr.records_of(data)[2]
        for r, col in mr.deferred_of(records):
            try:
                float(mr.field_text(records[r][2][col]))
            except ValueError:
                refused += 1
        assert refused, what
        with pytest.raises(ValueError):
            passages.sort_records(passages.read_matches(path))
    else:
        check_parity(path, writer_made=False)
    return mf


# ---- doubles through the kernel -------------------------------------------------------------

# tests/test_matches_host.py: test_hand_list
HAND = ("0.0", "-0.0", "5e-324", "2.2250738585072014e-308", "2.225073858507201e-308",
        "1.7976931348623157e+308", "1e23", "9007199254740993.0", "8.41e21", "1e-400",
        "1e400", "nan", "inf", "-inf", "", "-1e400", "-1e-400", "2.4703282292062327e-324",
        "2.4703282292062328e-324", "17976931348623159e292", "0.000", "1E5", "1e+05",
        "007.50", "12345678901234567", "0.00000000000000000000012345678901234567")
# ... test_off_grammar_strings_carry_no_value, those a bare field can hold
OFF_GRAMMAR = ("1_0", " 1.0", "+1.0", "0x1p3", "1.", ".5e", "Infinity", "1.0 ", ".5", "-", "e5",
               "1e", "1e+", "-nan", "NaN", "INF", "--1", "1..0", "1e5.0", "123456789012345678",
               "1.23456789012345678", "0.100000000000000000000",
               "1234567890123456789012345678901234567890")


def float_accepts(text):
    try:
        float(text)
        return True
    except ValueError:
        return False


def tie_texts():
    """Decimal strings of at most 17 significant digits that lie exactly half way between two
    doubles, with their decimal neighbours.  Half way between neighbours of spacing 2^s is
    odd * 2^(s-1) with odd in [2^53, 2^54); written w * 10^q that needs 5^q | odd for q >= 0
    (every q of 0..23 and every s - 1 >= q for which w keeps 17 digits), and for q = -1 it is
    M + 0.5 (q <= -2 takes 18 digits).  Each once as w.0e(q) (q one lower in the kernel) where
    17 digits allow, once as w e(q)."""
    out = []
    for q in range(0, 24):
        p5 = 5 ** q
        k_lo, k_hi = -(-(1 << 53) // p5) | 1, ((1 << 54) - 1) // p5
        k_hi -= 1 - k_hi % 2
        for k in sorted({k_lo, k_hi}):
            if not (1 << 53) <= k * p5 < (1 << 54):
                continue
            t = q                                   # the power of two: s - 1
            while k << (t - q) < 10 ** 17:
                w = k << (t - q)
                assert float(w * 10 ** q) in (float((k * p5 - 1) << t), float((k * p5 + 1) << t))
                for v in (w - 1, w, w + 1):
                    if len(str(v)) <= 16:
                        out.append("%d.0" % v if q == 0 else "%d.0e+%02d" % (v, q))
                    out.append("%de0" % v if q == 0 else "%de+%02d" % (v, q))
                t += 1
    for m in ((1 << 52), (1 << 52) + 1, (1 << 52) + 2, (1 << 53) - 2, (1 << 53) - 1, 6 << 50):
        out += ["%d.5" % m, "%d.4" % m, "%d.6" % m, "%d.5e0" % m, "-%d.5" % m]
    return out


def special_texts():
    sub = [repr(k * 5e-324) for k in range(1, 65)]
    top_sub = 2.0 ** -1022 * (1 - 2.0 ** -52)
    sub += [repr(float(x)) for x in (np.nextafter(top_sub, 0.0), top_sub, 2.0 ** -1022,
                                     np.nextafter(2.0 ** -1022, 1.0))]
    sub += ["2.4703282292062327e-324", "2.4703282292062328e-324"]
    top = ["1.7976931348623157e+308", "1.7976931348623158e+308", "1.7976931348623159e+308",
           "17976931348623158e292", "17976931348623159e292", "-1.7976931348623159e+308"]
    forms = ["1E5", "1e+05", "007.50", "0.000", "-0.0", "-0", "1e5", "1e05", "1e005", "1e0005",
             "1e00005", "1e000005", "1e-400", "1e400", "0e999999", "1e-999999", "1e999999",
             "-0e-999999", "0" * 25 + "12345678901234567", "0." + "0" * 25 + "12345678901234567",
             "-" + "0" * 25 + ".12345678901234567e-5"]
    return sub + top + forms


@functools.lru_cache(maxsize=None)
def random_texts():
    """repr of 200 000 finite doubles of random bit patterns (the host test's seed)."""
    v = np.random.default_rng(20211).integers(0, 1 << 64, 210_000, dtype=np.uint64).view(np.float64)
    v = v[np.isfinite(v)][:200_000]
    assert len(v) == 200_000
    texts = [repr(x) for x in v.tolist()]
    return texts, np.array([float(t) for t in texts], dtype=np.float64).view(np.uint64)


def check_doubles(tmp_path, texts, want=None):
    """The texts in columns 9 and 11, two per row; MatchFile's values against float()."""
    texts = list(texts) + ["0.5"] * (len(texts) % 2)
    raw = [t.encode() for t in texts]
    data = b"".join(plain_row(k, k + 1000, dist=raw[2 * k], comb=raw[2 * k + 1])
                    for k in range(len(raw) // 2))
    if want is None:
        want = np.array([float(t) if t else float("nan") for t in texts], dtype=np.float64).view(np.uint64)
    deferred = sum(1 for t in raw if not mr.distance_is_plain(t))
    with MatchFile(write(tmp_path, "d.csv", data)) as mf:
        assert not mf.outside and mf.n == len(raw) // 2
        assert mf.n_deferred == deferred
        assert mf.status == (abi.FS_MATCHES_DEFERRED if deferred else abi.FS_MATCHES_PARSED)
        got = np.stack([mf.dist, mf.comb], axis=1).reshape(-1).view(np.uint64)
    wrong = np.flatnonzero(got != want)
    assert len(wrong) == 0, [(texts[k], hex(int(got[k])), hex(int(want[k]))) for k in wrong[:5]]
    return deferred


def test_doubles_of_random_bit_patterns(tmp_path, stage):
    texts, want = random_texts()
    assert check_doubles(tmp_path, texts, want) == 0


def test_doubles_by_hand_ties_subnormals_and_the_top(tmp_path, stage):
    ties = tie_texts()
    assert len(ties) > 3000
    assert check_doubles(tmp_path, list(HAND) + ties + special_texts()) == 0


def test_doubles_float_reads_and_the_kernel_leaves_alone(tmp_path, stage):
    planted = [t for t in OFF_GRAMMAR if float_accepts(t)]
    assert len(planted) >= 12
    assert check_doubles(tmp_path, list(HAND) + planted + special_texts()) == len(planted)


# ---- every refusal at every edge ------------------------------------------------------------

BEHIND = b",11,8,s,22,ANNA,1,0.5,3,0.25\r\n"
LAST_HEAD = b"edge.txt,7,w,11,8,s,22,ANNA,1,0.5,3,"


def planted(off, field, at):
    """A file whose column 2 of one row is `field`, field[at] at absolute offset `off`."""
    head = b"edge.txt,7,"
    data = padding(off - at - len(head)) + head + field + BEHIND + sized_row(60) * 2
    return data


def at_the_start(field):
    return field + b",7,w" + BEHIND + sized_row(60) * 2


def at_the_end(field):
    """... the last field of a last row without a terminator."""
    return sized_row(60) * 3 + LAST_HEAD + field


def sweep(length):
    return [e + d for e in EDGES for d in range(-length - 3, 4)]


def starts(field, at):
    """`field` as the file's first field, field[at] at offset 0..3 where a bare field allows."""
    if field[:1] == b'"':
        return [("start %d" % at, at_the_start(field))]
    return [("start %d" % k, at_the_start(field[at - k:] if k < at else b"a" * (k - at) + field))
            for k in range(4)]


# (field, where the planted bytes begin in it, their number); b"a"/b"b" stand on either side
def bare(payload):
    return b"a" + payload + b"b", 1, len(payload)


REFUSALS = {
    "quote_in_bare_field": bare(b'"'),
    "text_behind_closing_quote": (b'"ab"c', 0, 5),
    "lone_cr": bare(b"\r"),
    "nul": bare(b"\x00"),
    "stray_continuation": bare(b"\x80"),
    "cut_2_after_1": bare(b"\xc3"),
    "cut_3_after_1": bare(b"\xe4"),
    "cut_3_after_2": bare(b"\xe4\xb8"),
    "cut_4_after_1": bare(b"\xf0"),
    "cut_4_after_2": bare(b"\xf0\x9f"),
    "cut_4_after_3": bare(b"\xf0\x9f\x98"),
    "overlong_c0_af": bare(b"\xc0\xaf"),
    "overlong_e0_80_80": bare(b"\xe0\x80\x80"),
    "surrogate_ed_a0_80": bare(b"\xed\xa0\x80"),
    "overlong_f0_80_80_80": bare(b"\xf0\x80\x80\x80"),
    "beyond_f4_90_80_80": bare(b"\xf4\x90\x80\x80"),
    "f5": bare(b"\xf5"),
}
REFUSAL_BITS = {"quote_in_bare_field": mr.BAD_OPEN | mr.BAD_CLOSE,
                "text_behind_closing_quote": mr.BAD_CLOSE, "lone_cr": mr.BAD_CR,
                "nul": mr.BAD_NUL}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_a_refusal_at_every_edge(tmp_path, stage, case):
    field, at, length = REFUSALS[case]
    files = [("offset %d" % off, planted(off, field, at)) for off in sweep(length)]
    files += starts(field, at)
    # the last bytes: nothing behind the planted ones
    files.append(("end", at_the_end(field[:at + length])))
    for what, data in files:
        if what.startswith("offset"):
            off = int(what.split()[1])
            assert data[off:off + length] == field[at:at + length]
        mf = assert_verdict(tmp_path, data, (case, what))
        assert mf.outside and mf.reason & REFUSAL_BITS.get(case, mr.BAD_UTF8), (case, what, mf.reason)


# valid twins: (field of column 2, where the bytes begin, their number, the same at the file's
# end as a distance field float() reads: a digit of as many bytes)
TWINS = {
    "quote_pair_in_quotes": (b'"a""b"', 2, 2, None),
    "crlf_in_quotes": (b'"a\r\nb"', 2, 2, None),
    "two_bytes": ("aéb".encode(), 1, 2, "0.2٥".encode()),
    "three_bytes": ("a中b".encode(), 1, 3, "0.2５".encode()),
    "four_bytes": ("a\U0001f600b".encode(), 1, 4, "0.2\U0001d7d3".encode()),
    "closing_quote": (b'"ab"', 3, 1, b'"0.25"'),
}


@pytest.mark.parametrize("case", sorted(TWINS))
def test_a_valid_twin_at_every_edge(tmp_path, stage, case):
    field, at, length, last = TWINS[case]
    files = [("offset %d" % off, planted(off, field, at)) for off in sweep(length)]
    files += starts(field, at)
    if last is not None:
        files.append(("end", at_the_end(last)))
    for what, data in files:
        mf = assert_verdict(tmp_path, data, (case, what))
        assert not mf.outside, (case, what, mf.reason)
        if what == "end":
            assert mf.n_deferred == 1 and mf.comb[-1] == 0.25


@pytest.mark.parametrize("size", [TILE - 1, TILE, TILE + 1])
def test_the_file_ends_at_a_tile_edge(tmp_path, stage, size):
    """The final CRLF before, across and on the edge; then the same sizes with no terminator."""
    data = padding(size)
    assert len(data) == size and data.endswith(b"\r\n")
    rows = check_parity(write(tmp_path, "crlf.csv", data), False).n
    bare_end = padding(size + 2)[:-2]
    assert len(bare_end) == size
    assert check_parity(write(tmp_path, "bare.csv", bare_end), False).n == rows
    quoted_end = padding(size - len(LAST_HEAD) - 6) + LAST_HEAD + b'"0.25"'
    assert len(quoted_end) == size
    assert_verdict(tmp_path, quoted_end)


# ---- structure -----------------------------------------------------------------------------

def short_rows(n):
    return [row("w%d" % (k // 50), k, k + 9, "f", "s", "C", 1, 0.5, 1, 0.25) for k in range(n)]


def test_a_quoted_field_longer_than_a_tile(tmp_path, stage):
    rows = short_rows(520)
    piece = 'ab,"c"\r\nde,\n""f\r'
    rows[420][2] = (piece * (20000 // len(piece) + 1))[:20000]
    data = csv_bytes(rows)
    at = data.index(b'"ab,')
    assert at // TILE + 2 <= (at + 20000) // TILE      # a tile in between holds no row start
    check_parity(write(tmp_path, "long.csv", data), False)


def test_a_row_longer_than_the_stage_among_short_ones(tmp_path, stage):
    rows = short_rows(200)
    assert len(csv_bytes(rows[:1])) <= 40
    for k, n in ((70, 9000), (130, 8150), (199, 9000)):
        rows[k][5] = "y" * n
    check_parity(write(tmp_path, "row9000.csv", csv_bytes(rows)), False)


@pytest.mark.parametrize("stretch", [8191, 8192, 8193])
def test_a_wave_s_stretch_around_the_stage_size(tmp_path, stage, stretch):
    """Rows 64..127 are the second wave's: it stages from row 63's start, rounded down to 16,
    to row 128's start.  That stretch at 8191, 8192 and 8193 bytes, row 63 at every offset
    mod 16."""
    for lead in range(16):
        front = sized_row(48) * 62 + sized_row(48 + lead)                   # rows 0..62
        assert len(front) % 16 == lead
        body = stretch - lead                                               # rows 63..127
        mid = sized_row(100) * 64 + sized_row(body - 6400)
        data = front + mid + sized_row(48) * 9
        starts = [0]
        for line in data.split(b"\r\n")[:-1]:
            starts.append(starts[-1] + len(line) + 2)
        assert starts[128] - (starts[63] & ~15) == stretch and starts[63] & 15 == lead
        mf = check_parity(write(tmp_path, "wave.csv", data), False)
        assert mf.n == 137


def test_the_quoting_parity_over_the_scan_s_chunk(tmp_path, stage):
    """1026 tiles.  Tiles 0..1021 are one block of whole rows repeated (a quoted field with
    commas in each: an even count).  A quoted field opens in tile 1022 and closes in tile
    1025, CRLFs inside it all the way: tiles 1023 and 1024, the last of the scan's first chunk
    and the first of its second, start inside quotes.  The Python reader parses the block once
    and the rest once; the whole file's reference is put together from the two."""
    block = sized_row(128) * 60 + b'q.txt,7,"a,b",1,9,%s,2,A,1,0.125,3,1e-05\r\n' % (b"s" * 88) + \
        sized_row(128) * 67
    assert len(block) == TILE
    piece = "line one,\r\nline \"\"two\"\"\r\n"
    long_field = (piece * 2000)[:45000]
    rest = csv_bytes([row("r.txt", 1, 2, "x" * 7900), row("r.txt", 2, 3, long_field),
                      row("r.txt", 3, 4, "tail"), row("r.txt", 4, 5, "é")]) + sized_row(128) * 3
    data = block * 1022 + rest
    assert (len(data) + TILE - 1) // TILE == 1026
    opens = 1022 * TILE + rest.index(b'"line')
    closes = opens + rest[rest.index(b'"line'):].index(b'",11,')
    assert opens // TILE == 1022 and closes // TILE == 1025
    for t in (1023, 1024):
        assert b"\r\n" in data[t * TILE:(t + 1) * TILE]
    block_rows = passages.read_matches(write(tmp_path, "block.csv", block))
    rest_rows = passages.read_matches(write(tmp_path, "rest.csv", rest))
    nb, n = len(block_rows), 1022 * len(block_rows) + len(rest_rows)
    assert nb == 128 and len(rest_rows) == 7

    def column(col, conv, dtype):
        b = np.array([conv(r[col]) for r in block_rows], dtype=dtype)
        return np.concatenate([np.tile(b, 1022), np.array([conv(r[col]) for r in rest_rows], dtype=dtype)])

    with MatchFile(write(tmp_path, "chunk.csv", data)) as mf:
        assert not mf.outside and mf.n == n and mf.n_deferred == 0 and not mf.has_header
        assert np.array_equal(mf.fan, column(1, int, np.uint32))
        assert np.array_equal(mf.orig, column(4, int, np.uint32))
        assert np.array_equal(mf.lev, column(10, int, np.uint32))
        for got, col in ((mf.dist, 9), (mf.comb, 11)):
            assert np.array_equal(got.view(np.uint64), column(col, passages._distance, np.float64).view(np.uint64))
        assert mf.names == ["p", "q.txt", "r.txt"]
        pick = np.concatenate([np.random.default_rng(5).integers(0, n, 980),
                               np.arange(n - 10, n), 60 + nb * np.arange(0, 1022, 103)])
        assert len(pick) == 1000
        for col in (0, 2, 5, 11):
            want = [(block_rows[k % nb] if k < 1022 * nb else rest_rows[k - 1022 * nb])[col]
                    for k in pick.tolist()]
            assert mf.text(col, pick) == want, col


# ---- the deferred list's bound --------------------------------------------------------------

@pytest.mark.parametrize("n_rows,bound", [(5000, 4096), (80_000, 5000)])
def test_the_deferred_list_on_and_above_its_bound(tmp_path, stage, n_rows, bound):
    assert bound == max(4096, n_rows // 16)

    def with_deferred(count):                       # `count` distance fields spelt +0.5
        return b"".join(plain_row(k, k + 1000, dist=b"+0.5" if 2 * k < count else b"0.25",
                                  comb=b"+0.5" if 2 * k + 1 < count else b"0.125")
                        for k in range(n_rows))

    with MatchFile(write(tmp_path, "on.csv", with_deferred(bound))) as mf:
        assert mf.status == abi.FS_MATCHES_DEFERRED and not mf.outside
        assert mf.n == n_rows and mf.n_deferred == bound
        k = np.arange(n_rows)
        assert np.array_equal(mf.dist, np.where(2 * k < bound, float("+0.5"), 0.25))
        assert np.array_equal(mf.comb, np.where(2 * k + 1 < bound, float("+0.5"), 0.125))
    data = with_deferred(bound + 1)
    assert mr.verdict(data)[:2] == (True, mr.BAD_DEFER)
    path = write(tmp_path, "above.csv", data)
    with MatchFile(path) as mf:
        assert mf.outside and mf.status == abi.FS_MATCHES_OUTSIDE
        assert mf.reason == abi.FS_MATCH_BAD_DEFER
    assert both_readers(tmp_path, "passages", path)[0][1].count(b"\r\n") >= 2


# ---- mutants --------------------------------------------------------------------------------

@pytest.mark.parametrize("part", range(4))
def test_mutants(tmp_path, stage, part):
    """400 single-byte changes per stage setting of a good file of three tiles, a quarter of
    them per case (their spread over inside, outside and the reasons is asserted by
    tests/test_matches_restated_host.py)."""
    assert_verdict(tmp_path, mr.base_file(), "base")
    for what, data in mr.mutants(stage)[part::4]:
        assert_verdict(tmp_path, data, what)
