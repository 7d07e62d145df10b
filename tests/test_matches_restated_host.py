"""tests/matches_restated.py held to Python itself, without a GPU: on every mutant of
tests/test_gpu_matches_edges.py and every hand case of tests/test_gpu_matches.py its UTF-8 bit
is bytes.decode's verdict, and where it says "inside" its rows and fields are csv.reader's, its
header flag is the Python reader's and its deferred fields are those the documented distance
grammar refuses.  The spread of the mutant set is asserted here too, so that it is known to
hold before any GPU run."""

import csv
import io

import pytest

from fandom_search_amd import abi
from tests import matches_restated as mr
from tests.test_gpu_matches import FIELDS, csv_bytes, odd_rows, off_grammar_files, some_rows

STAGES = ("0", "1")


def python_rows(data):
    """(has_header, records) as passages.read_matches takes them from the bytes."""
    rows = [r for r in csv.reader(io.StringIO(data.decode("utf-8"), newline="")) if r]
    header = bool(rows) and rows[0] == FIELDS
    return header, rows[1:] if header else rows


def check_against_python(data):
    """The restatement of `data` against decode and csv.reader; returns the verdict."""
    v = mr.verdict(data)
    outside, reason, header, n_rows, n_deferred = v
    try:
        data.decode("utf-8")
        decodes = True
    except UnicodeDecodeError:
        decodes = False
    assert bool(mr.records_of(data)[0] & mr.BAD_UTF8) == (not decodes)
    assert outside == bool(reason) and (decodes or reason == reason & mr.BYTE_BITS)
    if outside and reason != mr.BAD_DEFER:
        return v
    want_header, want = python_rows(data)
    assert mr.text_rows(data) == want
    assert header == want_header and n_rows == len(want)
    # a quoted distance field is of another shape whatever it holds: its bytes begin with '"'
    raw = mr.records_of(data)[2]
    refused = sum(1 for (_, _, f), r in zip(raw, want) for col in mr.DISTANCE_COLUMNS
                  if f[col][:1] == b'"' or not mr.distance_is_plain(r[col].encode()))
    assert n_deferred == refused
    return v


def test_the_constants_are_the_header_s():
    for name in ("PARSED", "DEFERRED", "OUTSIDE"):
        assert getattr(mr, name) == getattr(abi, "FS_MATCHES_" + name)
    for name in ("NUL", "OPEN", "CLOSE", "CR", "FIELDS", "INT", "UTF8", "ROW", "DEFER"):
        assert getattr(mr, "BAD_" + name) == getattr(abi, "FS_MATCH_BAD_" + name)
    assert mr.FIELDS == FIELDS and mr.N_FIELDS == abi.FS_MATCH_FIELDS


@pytest.mark.parametrize("header", [False, True])
@pytest.mark.parametrize("terminator", ["\r\n", "\n"])
def test_odd_rows_are_inside(header, terminator):
    data = csv_bytes(odd_rows(), header, terminator)
    v = check_against_python(data)
    assert v == (False, 0, header, len(odd_rows()), 0)
    assert check_against_python(data[:-len(terminator)]) == v      # no last terminator


@pytest.mark.parametrize("name,reason,data", off_grammar_files(),
                         ids=lambda v: v if isinstance(v, str) else "")
def test_hand_cases(name, reason, data):
    v = check_against_python(data)
    if name == "distance_float_refuses":          # float() refuses it on the host, later
        assert v == (False, 0, False, 6, 1)
    elif name == "quoted_header":                 # not the header byte for byte: a record
        assert v[:2] == (True, mr.BAD_INT)
    else:
        assert v[:2] == (True, reason), name


def test_small_files():
    header = csv_bytes([], True)
    for data, want in ((b"", (False, 0, False, 0, 0)), (b"\r\n\n\r\n", (False, 0, False, 0, 0)),
                       (header, (False, 0, True, 0, 0)), (header[:-2], (False, 0, True, 0, 0)),
                       (b"\n" + header + b"\n", (False, 0, True, 0, 0)),
                       (header + header, (True, mr.BAD_INT, True, 0, 0)),
                       (b'""\n', (True, mr.BAD_FIELDS, False, 0, 0)),
                       (b"\r", (True, mr.BAD_CR, False, 0, 0)),
                       (b'"', (True, mr.BAD_CLOSE, False, 0, 0)),
                       (b'"a"\rb\n', (True, mr.BAD_CR, False, 0, 0)),
                       (b'a"b"\n', (True, mr.BAD_OPEN, False, 0, 0)),
                       (b'a"b\n', (True, mr.BAD_OPEN | mr.BAD_CLOSE, False, 0, 0))):
        assert check_against_python(data) == want, data


def test_the_distance_grammar_is_fs_dec_s_on_the_host_lists():
    """The regular expression and fs_matches_parse_double agree on which strings are whose
    (the lists of tests/test_matches_host.py and a few more)."""
    from fandom_search_amd.matches import parse_double
    mine = ["0.0", "-0.0", "5e-324", "1e23", "9007199254740993.0", "1e-400", "1e400", "nan",
            "inf", "-inf", "", "0.000", "1E5", "1e+05", "007.50", "12345678901234567",
            "0.00000000000000000000012345678901234567", "0e999999", "1e-999999", "-0",
            "00000000000000000000000001.2345678901234567"]
    other = ["1_0", " 1.0", "+1.0", "0x1p3", "1.", ".5e", "Infinity", "1,0", "1.0 ", ".5", "-",
             "e5", "1e", "1e+", "-nan", "NaN", "INF", "--1", "1..0", "1e5.0", "123456789012345678",
             "1.23456789012345678", "0.100000000000000000000", '"0.5"', "1e5\n", "0.5\n", "١"]
    for text in mine:
        assert mr.distance_is_plain(text.encode()) and parse_double(text)[0] == abi.FS_DEC_SURE
    for text in other:
        assert not mr.distance_is_plain(text.encode()), text
        assert parse_double(text)[0] == abi.FS_DEC_NOT_MINE, text


@pytest.mark.parametrize("stage", STAGES)
def test_mutants_and_their_spread(stage):
    base = mr.base_file()
    assert 2 * 16384 + 2048 < len(base) < 3 * 16384
    assert check_against_python(base) == (False, 0, True, 30 + 410, 0)
    base_ends = mr.field_ends(base)
    muts = mr.mutants(stage)
    assert len(muts) == mr.MUTANTS and len(set(d for _, d in muts)) > mr.MUTANTS * 3 // 4
    inside = outside = moved = 0
    bits = dict.fromkeys(("NUL", "OPEN", "CLOSE", "CR", "FIELDS", "INT", "UTF8"), 0)
    for what, data in muts:
        v = check_against_python(data)
        if v[0]:
            outside += 1
            for name in bits:
                bits[name] += bool(v[1] & getattr(mr, "BAD_" + name))
        else:
            inside += 1
            moved += mr.field_ends(data) != base_ends
    assert inside * 4 >= mr.MUTANTS and outside * 4 >= mr.MUTANTS, (inside, outside)
    assert min(bits.values()) >= 10, bits
    assert moved >= 30, moved


def test_mutant_positions_sit_at_the_edges():
    import numpy as np
    n = len(mr.base_file())
    pos = mr.mutant_positions(np.random.default_rng(1), n, 400)
    near = [min(min(p % e, e - p % e) for e in mr.EDGES) <= 4 or p <= 4 or p >= n - 5
            for p in pos[200:]]
    assert all(near)
    for e in (4096, 16384, 32768):
        assert any(abs(p - e) <= 4 for p in pos[200:]), e
    assert any(p <= 4 for p in pos[200:]) and any(p >= n - 5 for p in pos[200:])


def test_some_rows_round_trip():
    data = csv_bytes(some_rows(40), True, "\n")
    assert check_against_python(data) == (False, 0, True, 40, 0)
