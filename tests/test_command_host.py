"""The host layer the analysis commands share (fandom_search_amd/command.py), the dispatcher of
cli.py and the command line's surface, without a GPU: the library and the match reader are
stood in for."""

import argparse
import csv
import ctypes as C
import json
import os

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, command, matches
from fandom_search_amd.passages import _CHAR, _ORIG_WORD, _SCENE
from tests.golden import make_cli_surface

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32)])


# ---- grow ----------------------------------------------------------------------------------

class FakeCall:
    """A library call with `total` records to give: FS_E_CAPACITY and the count while the buffer
    is smaller, else the records; or `code` whatever the buffer."""

    def __init__(self, total, code=abi.FS_OK):
        self.total, self.code, self.caps = total, code, []

    def __call__(self, buf, cap, got):
        self.caps.append(cap)
        if self.code != abi.FS_OK:
            return self.code
        got._obj.value = self.total
        if cap < self.total:
            return abi.FS_E_CAPACITY
        out = np.ctypeslib.as_array((C.c_uint32 * (2 * cap)).from_address(buf.value))
        out[:2 * self.total] = np.arange(2 * self.total, dtype=np.uint32)
        return abi.FS_OK


def test_grow_repeats_the_call_once_with_the_reported_count():
    call = FakeCall(7)
    out = command.grow(call, DTYPE, 3)
    assert call.caps == [3, 7]
    assert out.dtype == DTYPE and len(out) == 7
    assert out["a"].tolist() == list(range(0, 14, 2)) and out["b"].tolist() == list(range(1, 14, 2))


def test_grow_calls_once_when_the_records_fit():
    call = FakeCall(7)
    assert len(command.grow(call, DTYPE, 4096)) == 7
    assert call.caps == [4096]
    call = FakeCall(0)
    assert len(command.grow(call, DTYPE, 0)) == 0 and call.caps == [0]


def test_grow_raises_any_other_code_after_one_call(monkeypatch):
    class Lib:
        fs_strerror = staticmethod(lambda rc: b"invalid argument")
        fs_last_error = staticmethod(lambda: b"min_words must be at least 1")
    monkeypatch.setattr(_lib, "load", lambda: Lib)
    call = FakeCall(7, abi.FS_E_INVALID)
    with pytest.raises(_lib.FsError) as e:
        command.grow(call, DTYPE, 3, "fs_fake")
    assert call.caps == [3] and e.value.code == abi.FS_E_INVALID
    assert str(e.value) == ("fs_fake failed: %d (invalid argument: min_words must be at least 1)"
                            % abi.FS_E_INVALID)


def test_grow_with_two_outputs_enlarges_only_the_one_that_was_short():
    seen = []

    def call(p, cap_p, got_p, q, cap_q, got_q):
        seen.append((cap_p, cap_q))
        got_p._obj.value, got_q._obj.value = 5, 2
        return abi.FS_E_CAPACITY if cap_p < 5 or cap_q < 2 else abi.FS_OK
    p, q = command.grow(call, [DTYPE, np.dtype(np.uint64)], [4, 16])
    assert seen == [(4, 16), (5, 16)]
    assert (len(p), p.dtype, len(q), q.dtype) == (5, DTYPE, 2, np.dtype(np.uint64))


# ---- the small helpers ------------------------------------------------------------------------

def test_n_script_of_and_work_names():
    assert command.n_script_of(np.array([], dtype=np.int64)) == 0
    assert command.n_script_of(np.array([3, 9, 0])) == 10
    rows = [["b.txt", "0"], ["a.txt", "1"], ["b.txt", "2"]]
    assert command.work_names(rows) == ["b.txt", "a.txt"] and command.work_names([]) == []


def test_prefixed():
    assert command.prefixed("runs/m.csv", None, ("-x.csv", "-x-y.csv")) == ("runs/m-x.csv",
                                                                             "runs/m-x-y.csv")
    assert command.prefixed("batch", None, ("-x.csv",)) == ("batch-x.csv",)
    assert command.prefixed("m.csv", "out/p", ("-x.csv",)) == ("out/p-x.csv",)


class LabelFile:
    """mf.labels of a MatchFile: {script word: label} per column, or None for a column."""

    def __init__(self, cols):
        self.cols, self.asked = cols, []

    def labels(self, column, n_script):
        self.asked.append((column, n_script))
        return self.cols[column]


def test_script_labels():
    cols = {_ORIG_WORD: {0: "may", 4: "force"}, _CHAR: {0: "BEN", 4: "HAN"},
            _SCENE: {0: "1, INT", 4: "2"}}
    mf = LabelFile(cols)
    assert command.script_labels(mf, 5) == {0: ("may", "BEN", "1, INT"), 4: ("force", "HAN", "2")}
    assert mf.asked == [(_ORIG_WORD, 5), (_CHAR, 5), (_SCENE, 5)]
    for column in cols:
        assert command.script_labels(LabelFile({**cols, column: None}), 5) is None
    assert command.script_labels(LabelFile({c: {} for c in cols}), 0) == {}


def test_write_tables(tmp_path):
    paths = [str(tmp_path / "a.csv"), str(tmp_path / "b.csv")]
    command.write_tables(paths, (["X", "Y"], ["Z"]), ([[1, "a,b"], [2, "line\nbreak"]], []))
    assert open(paths[0], "rb").read() == b'X,Y\r\n1,"a,b"\r\n2,"line\nbreak"\r\n'
    assert open(paths[1], "rb").read() == b"Z\r\n"
    command.write_tables(paths[:1], (["X"],), ([["café"]],))
    assert open(paths[0], "rb").read() == "X\r\ncafé\r\n".encode("utf-8")


# ---- run --------------------------------------------------------------------------------------

HEADS = (["A", "B"], ["C"])
FIELDS = ["f.txt", "0", "may", "", "0", "may", "", "BEN", "1", "0.0", "", "0.0"]


class FakeMatchFile:
    opened = []
    outside = False

    def __init__(self, path, device=0):
        FakeMatchFile.opened.append((path, device))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        FakeMatchFile.opened.append("closed")


@pytest.fixture
def ran(tmp_path, monkeypatch):
    """run over a one-record match file with tables that say who was asked; gives
    (reader, outside, device_body) -> (calls, outs)."""
    src = tmp_path / "m.csv"
    with open(src, "w", newline="", encoding="utf-8") as fh:
        csv.writer(fh).writerow(FIELDS)
    outs = (str(tmp_path / "o-a.csv"), str(tmp_path / "o-b.csv"))
    monkeypatch.setattr(matches, "MatchFile", FakeMatchFile)

    def go(reader, outside=False, device_body=([[1, 2]], [[3]])):
        calls = []
        FakeMatchFile.opened, FakeMatchFile.outside = [], outside
        monkeypatch.setattr(matches, "reader_of", lambda args: reader)

        def tables(rows, *opts):
            calls.append(("tables", rows, opts))
            return [["p", "q"]], [["r"], ["s"]]

        def tables_device(mf, *opts):
            calls.append(("tables_device", type(mf), opts))
            return device_body
        args = argparse.Namespace(matches=str(src), device=3, reader=None)
        got = command.run(args, HEADS, outs, tables, tables_device, (6, 0, 3))
        assert got is outs
        return calls, [list(csv.reader(open(p, newline="", encoding="utf-8"))) for p in outs]
    return go


def test_run_takes_the_device_tables(ran):
    calls, files = ran("device")
    assert calls == [("tables_device", FakeMatchFile, (6, 0, 3))]
    (path, device), closed = FakeMatchFile.opened
    assert path.endswith("m.csv") and device == 3 and closed == "closed"
    assert files == [[["A", "B"], ["1", "2"]], [["C"], ["3"]]]


def test_run_falls_back_for_a_file_outside_the_device_grammar(ran):
    calls, files = ran("device", outside=True)
    assert calls == [("tables", [FIELDS], (6, 0, 3))]
    assert FakeMatchFile.opened[-1] == "closed"
    assert files == [[["A", "B"], ["p", "q"]], [["C"], ["r"], ["s"]]]


def test_run_falls_back_when_the_device_tables_are_none(ran):
    calls, files = ran("device", device_body=None)
    assert [c[0] for c in calls] == ["tables_device", "tables"]
    assert calls[1] == ("tables", [FIELDS], (6, 0, 3))
    assert files == [[["A", "B"], ["p", "q"]], [["C"], ["r"], ["s"]]]


def test_run_under_the_python_reader_opens_no_match_file(ran):
    calls, files = ran("python")
    assert calls == [("tables", [FIELDS], (6, 0, 3))] and FakeMatchFile.opened == []
    assert files == [[["A", "B"], ["p", "q"]], [["C"], ["r"], ["s"]]]


# ---- the command line's surface ------------------------------------------------------------

def test_cli_surface_is_the_committed_one():
    with open(os.path.join(GOLDEN, "cli_surface.json"), encoding="utf-8") as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(make_cli_surface.surface(cli.build_parser())))
    assert [s[0] for s in got] == [s[0] for s in want]
    for mine, theirs in zip(got, want):
        assert mine == theirs, mine[0]


# ---- the dispatcher ------------------------------------------------------------------------

SPANS = "--min-words must be at least 1, --max-gap at least 0"
WORKS = "--min-words and --min-works must be at least 1, --max-gap at least 0"
STEPS = ("--min-words, --min-works, --min-steps and --min-step-works must be at least 1, "
         "--max-gap at least 0")
SHARE = "--min-share must be from 0 to 100"
REFUSED = [
    ("passages", ["m.csv", "--min-words", "0"], SPANS),
    ("passages", ["m.csv", "--max-gap", "-1"], SPANS),
    ("groups", ["m.csv", "meta.csv", "--min-words", "0"], WORKS),
    ("groups", ["m.csv", "meta.csv", "--min-works", "0"], WORKS),
    ("groups", ["m.csv", "meta.csv", "--max-gap", "-1"], WORKS),
    ("groups", ["m.csv", "meta.csv", "--by", "decade"],
     "--by takes year, month, author, language, tag or tag:<Category>, not 'decade'"),
    ("groups", ["m.csv", "meta.csv", "--by", "tag:"],
     "--by takes year, month, author, language, tag or tag:<Category>, not 'tag:'"),
    ("transitions", ["m.csv", "--min-words", "0"], STEPS),
    ("transitions", ["m.csv", "--min-works", "0"], STEPS),
    ("transitions", ["m.csv", "--min-steps", "0"], STEPS),
    ("transitions", ["m.csv", "--min-step-works", "0"], STEPS),
    ("transitions", ["m.csv", "--max-gap", "-1"], STEPS),
    ("transitions", ["m.csv", "--within", "-1"],
     "--within must be from 0 to 4294967294 (leave it out for any distance)"),
    ("transitions", ["m.csv", "--within", "4294967295"],
     "--within must be from 0 to 4294967294 (leave it out for any distance)"),
    ("transitions", ["m.csv", "--min-share", "101"], SHARE),
    ("transitions", ["m.csv", "--min-share", "-1"], SHARE),
    ("sources", ["a.csv", "b.csv", "-o", "x", "--min-words", "0"], SPANS),
    ("sources", ["a.csv", "b.csv", "-o", "x", "--max-gap", "-1"], SPANS),
    ("clusters", ["m.csv", "--min-size", "0"],
     "--min-words, --min-shared and --min-size must be at least 1, --max-gap at least 0"),
    ("clusters", ["m.csv", "--common", "0"],
     "--min-jaccard must be from 0 to 100, --common from 1 to 100"),
    ("variants", ["m.csv", "--top", "-1"], "--top must be at least 0, --min-records at least 1"),
    ("readings", ["m.csv", "--top", "-1"],
     "--min-words and --min-works must be at least 1, --max-gap and --top at least 0"),
    ("retellings", ["m.csv", "--min-passages", "0"],
     "--min-words and --min-passages must be at least 1, --max-gap at least 0"),
    ("companions", ["m.csv", "--min-both", "0"],
     "--min-words, --min-works and --min-both must be at least 1, --max-gap at least 0"),
]


@pytest.mark.parametrize("name,argv,message", REFUSED)
def test_a_value_out_of_range_ends_with_the_error_line(name, argv, message, monkeypatch):
    module = __import__("fandom_search_amd." + name, fromlist=[name])

    def process(args):
        raise AssertionError("process ran")
    monkeypatch.setattr(module, "process", process)
    with pytest.raises(SystemExit) as e:
        cli.main([name] + argv)
    assert e.value.code == "ao3.py %s: error: %s" % (name, message)


@pytest.mark.parametrize("name,argv", [
    ("passages", ["m.csv"]), ("groups", ["m.csv", "meta.csv"]), ("transitions", ["m.csv"]),
    ("sources", ["a.csv", "b.csv", "-o", "x"]), ("works", ["m.csv"])])
def test_a_value_error_of_the_command_ends_with_the_error_line(name, argv, monkeypatch):
    module = __import__("fandom_search_amd." + name, fromlist=[name])
    seen = []

    def process(args):
        seen.append(args)
        raise ValueError("script word 3 has two scenes, '1' and '2'")
    monkeypatch.setattr(module, "process", process)
    with pytest.raises(SystemExit) as e:
        cli.main([name] + argv)
    assert e.value.code == ("ao3.py %s: error: script word 3 has two scenes, '1' and '2'" % name)
    assert len(seen) == 1 and seen[0].min_words == 6 and seen[0].device == 0


def test_the_dispatcher_returns_what_process_returns(monkeypatch):
    from fandom_search_amd import pairs
    monkeypatch.setattr(pairs, "process", lambda args: ("ran", args.min_shared))
    args = cli.build_parser().parse_args(["pairs", "m.csv", "--min-shared", "9"])
    assert args.func(args) == ("ran", 9)
