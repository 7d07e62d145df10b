"""The match CSV reader without a GPU: its entry points are declared, exported and bound, the
dtypes mirror the header, and the number conversion the kernel applies
(fs_matches_parse_double, csrc/fs_dec.h) equals float() bit for bit on what repr writes and
refuses, without a value, what is not of its grammar."""

import ctypes as C
import os
import re
import struct

import numpy as np

from fandom_search_amd import _lib, abi
from fandom_search_amd.matches import parse_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("fs_matches_open", "fs_matches_read", "fs_matches_labels", "fs_matches_close",
                "fs_matches_parse_double")


def header_text():
    with open(os.path.join(ROOT, "include", "fandom_search.h")) as fh:
        return fh.read()


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    L = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name


def test_dtypes_match_the_header():
    text = header_text()
    assert "#define FS_MATCH_FIELDS 12" in text and abi.FS_MATCH_FIELDS == 12
    ix = abi.MATCH_IX_DTYPE
    assert ix.itemsize == 64 and ix.names == ("start", "end", "quoted", "head")
    assert [ix.fields[n][1] for n in ix.names] == [0, 8, 56, 60]
    assert ix.fields["end"][0].shape == (12,)
    body = re.search(r"typedef struct fs_match_ix \{(.*?)\} fs_match_ix;", text, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[FS_MATCH_FIELDS\])?;", body) == list(ix.names)
    assert abi.MATCH_DEFER_DTYPE.itemsize == 8 and abi.MATCH_DEFER_DTYPE.names == ("row", "col")
    assert C.sizeof(abi.FsMatchesInfo) == 96 and abi.FsMatchesInfo.ms.offset == 32
    body = re.search(r"typedef struct fs_matches_info \{(.*?)\} fs_matches_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[8\])?;", body) == [n for n, _ in abi.FsMatchesInfo._fields_]
    for name in ("FS_MATCHES_PARSED", "FS_MATCHES_DEFERRED", "FS_MATCHES_OUTSIDE",
                 "FS_MATCH_BAD_NUL", "FS_MATCH_BAD_OPEN", "FS_MATCH_BAD_CLOSE", "FS_MATCH_BAD_CR",
                 "FS_MATCH_BAD_FIELDS", "FS_MATCH_BAD_INT", "FS_MATCH_BAD_UTF8", "FS_MATCH_BAD_ROW",
                 "FS_MATCH_BAD_DEFER"):
        assert int(re.search(r"\b%s = (\d+)" % name, text).group(1)) == getattr(abi, name), name


def bits(x):
    return struct.pack("<d", x)


def assert_float(text):
    rc, got = parse_double(text)
    assert rc == abi.FS_DEC_SURE, text
    want = float(text) if text else float("nan")
    assert bits(got) == bits(want), (text, got, want)


def check_many(values):
    """repr of every value through the hook in one go (a call per value is Python's time)."""
    L = _lib.load()
    fn, out = L.fs_matches_parse_double, C.c_double(0.0)
    ref = C.byref(out)
    for x in values:
        raw = repr(x).encode()
        assert fn(raw, len(raw), ref) == abi.FS_DEC_SURE, raw
        if bits(out.value) != bits(float(raw)):
            raise AssertionError((raw, out.value))


def test_repr_of_a_million_random_bit_patterns():
    v = np.random.default_rng(20211).integers(0, 1 << 64, 1_000_000, dtype=np.uint64).view(np.float64)
    check_many(v[np.isfinite(v)].tolist())


def test_repr_of_distances():
    rng = np.random.default_rng(20231)
    check_many(rng.random(100_000).tolist())
    check_many([s * k * 2.0 ** -53 for k in range(0, 2000) for s in (1.0, -1.0)])
    check_many((rng.random(20_000) * 0.1 * rng.integers(0, 8, 20_000)).tolist())


def test_hand_list():
    for text in ("0.0", "-0.0", "5e-324", "2.2250738585072014e-308", "2.225073858507201e-308",
                 "1.7976931348623157e+308", "1e23", "9007199254740993.0", "8.41e21", "1e-400",
                 "1e400", "nan", "inf", "-inf", "", "-1e400", "-1e-400", "2.4703282292062327e-324",
                 "2.4703282292062328e-324", "17976931348623159e292", "0.000", "1E5", "1e+05",
                 "007.50", "12345678901234567", "0.00000000000000000000012345678901234567"):
        assert_float(text)
    assert bits(parse_double("-0.0")[1]) != bits(parse_double("0.0")[1])


def test_off_grammar_strings_carry_no_value():
    L = _lib.load()
    for text in ("1_0", " 1.0", "+1.0", "0x1p3", "1.", ".5e", "Infinity", "1,0", "1.0 ", ".5",
                 "-", "e5", "1e", "1e+", "-nan", "NaN", "INF", "--1", "1..0", "1e5.0",
                 "123456789012345678", "1.23456789012345678", "0.100000000000000000000",
                 "1234567890123456789012345678901234567890"):
        raw = text.encode()
        out = C.c_double(-123.25)
        assert L.fs_matches_parse_double(raw, len(raw), C.byref(out)) == abi.FS_DEC_NOT_MINE, text
        assert out.value == -123.25, text
        assert parse_double(text) == (abi.FS_DEC_NOT_MINE, None)
