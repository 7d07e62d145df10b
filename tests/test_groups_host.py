"""`ao3.py groups` without a GPU: the join of works to metadata rows, the keys of every --by,
the order of the groups, the oracle's known answers (every figure written out here), the
parser, the C ABI's declarations and the committed expected CSVs."""

import csv
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli, groups
from tests import groups_restated as gr
from tests import passages_restated as pr
from tests.golden import make_groups_golden as mgg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _meta_text(rows, fields=groups.META_FIELDS):
    buf = io.StringIO(newline="")
    w = csv.DictWriter(buf, fields, extrasaction="ignore")
    w.writeheader()
    for r in rows:
        w.writerow(dict(dict.fromkeys(fields, ""), **r))
    return buf.getvalue()


def _meta(tmp_path, rows, by="year", fields=groups.META_FIELDS):
    path = tmp_path / "meta.csv"
    path.write_text(_meta_text(rows, fields), newline="", encoding="utf-8")
    return groups.read_meta(str(path), by)


TAGS = json.dumps({"Rating": "General Audiences", "Relationship": "A/B; A & C; A/B",
                   "Additional Tags": "Fluff;  ; Slow; Burn; Fluff"})
ROWS = [dict(FILENAME="works/123.html", AUTHOR=" anna ", PUBLICATION_DATE="2016-02-29",
             LANGUAGE="English", TAGS=TAGS),
        dict(FILENAME="124.html", AUTHOR="AOOO_UNSPECIFIED", PUBLICATION_DATE="AOOO_UNSPECIFIED",
             LANGUAGE="", TAGS=json.dumps({"Rating": "Mature"})),
        dict(FILENAME="125.html", AUTHOR="", PUBLICATION_DATE="2016-2-9", LANGUAGE="Deutsch",
             TAGS="{}"),
        dict(FILENAME="999.html", AUTHOR="zed", PUBLICATION_DATE="2019-01-01",
             LANGUAGE="Italiano", TAGS=json.dumps({"Relationship": "X/Y"}))]


# ---- keys, stems and membership -----------------------------------------------------------

def test_stems_join_txt_to_html(tmp_path):
    assert groups.stem("fan/123.txt") == groups.stem("123.html") == "123" == gr.stem("a/123.txt")
    assert groups.stem("a.b.txt") == gr.stem("a.b.txt") == "a.b" and groups.stem("w1") == "w1"
    meta = _meta(tmp_path, ROWS)
    keys, off, grp, in_meta = groups.membership(["123.txt", "x/125.txt", "777.txt"], meta, "year")
    assert keys == ["2016", "2019", "(unknown date)", "(no metadata)"]
    assert off.tolist() == [0, 1, 2, 3] and grp.tolist() == [0, 2, 3]
    assert in_meta == [1, 1, 2, 0]                         # 999 was never searched: still counted


def test_every_by(tmp_path):
    a, b, c, _ = ROWS
    assert groups.keys_of(a, "year") == ["2016"] and groups.keys_of(a, "month") == ["2016-02"]
    assert groups.keys_of(b, "year") == groups.keys_of(c, "month") == ["(unknown date)"]
    assert groups.keys_of(a, "author") == ["anna"] and groups.keys_of(c, "author") == ["(empty)"]
    assert groups.keys_of(b, "author") == ["AOOO_UNSPECIFIED"]
    assert groups.keys_of(b, "language") == ["(empty)"]
    assert groups.keys_of(a, "tag") == ["Rating: General Audiences", "Relationship: A/B",
                                        "Relationship: A & C", "Additional Tags: Fluff",
                                        "Additional Tags: Slow", "Additional Tags: Burn"]
    assert groups.keys_of(a, "tag:Relationship") == ["A/B", "A & C"]
    assert groups.keys_of(b, "tag:Relationship") == ["(none)"]       # a missing category
    assert groups.keys_of(c, "tag") == ["(none)"]
    for row in ROWS:
        for by in ("year", "month", "author", "language", "tag", "tag:Relationship", "tag:None"):
            assert groups.keys_of(row, by) == gr.keys_of(row, by)
    for bad in ("", "[1]", '{"Rating": 3}', "Fluff"):
        row = dict(a, TAGS=bad)
        for f in (groups.keys_of, gr.keys_of):
            with pytest.raises(ValueError) as e:
                f(row, "tag")
            assert "works/123.html" in str(e.value)
    for bad in ("decade", "tag:", "Tag"):
        with pytest.raises(ValueError):
            groups.check_by(bad)


def test_group_order_and_works_in_meta(tmp_path):
    meta = _meta(tmp_path, ROWS, "tag")
    names = ["125.txt", "123.txt", "500.txt"]
    keys, off, grp, in_meta = groups.membership(names, meta, "tag")
    assert keys == ["Additional Tags: Burn", "Additional Tags: Fluff", "Additional Tags: Slow",
                    "Rating: General Audiences", "Rating: Mature", "Relationship: A & C",
                    "Relationship: A/B", "Relationship: X/Y", "(none)", "(no metadata)"]
    assert in_meta == [1, 1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert [grp[off[w]:off[w + 1]].tolist() for w in range(3)] == [[8], [0, 1, 2, 3, 5, 6], [9]]
    want = gr.membership(names, {gr.stem(r["FILENAME"]): r for r in meta.values()}, "tag")
    assert (keys, in_meta) == (want[0], want[2])
    assert [grp[off[w]:off[w + 1]].tolist() for w in range(3)] == want[1]
    keys, _, _, in_meta = groups.membership([], meta, "author")     # no work: the rows' groups
    # (empty) is a key like any other: only the three of LAST_GROUPS go behind the rest
    assert keys == ["(empty)", "AOOO_UNSPECIFIED", "anna", "zed"] and in_meta == [1, 1, 1, 1]


def test_duplicate_stems_and_missing_columns(tmp_path):
    with pytest.raises(ValueError) as e:
        _meta(tmp_path, ROWS + [dict(FILENAME="old/123.txt")])
    assert "'123'" in str(e.value)
    meta = _meta(tmp_path, ROWS)
    with pytest.raises(ValueError) as e:
        groups.membership(["a/77.txt", "b/77.html"], meta, "year")
    assert "'77'" in str(e.value)
    with pytest.raises(ValueError) as e:
        _meta(tmp_path, ROWS, fields=groups.META_FIELDS[1:])
    assert "FILENAME" in str(e.value)
    with pytest.raises(ValueError) as e:
        _meta(tmp_path, ROWS, "tag:Rating", fields=groups.META_FIELDS[:-1])
    assert "TAGS" in str(e.value)
    assert len(_meta(tmp_path, ROWS, "author", fields=groups.META_FIELDS[:-1])) == 4


# ---- oracle known answers -------------------------------------------------------------

def _diag(work, fan0, orig0, n, exact=1):
    return [(work, fan0 + k, orig0 + k, exact) for k in range(n)]


def _group(**kw):
    d = dict.fromkeys(gr.GROUP_KEYS, 0)
    d.update(peak_first=gr.NONE, top_label=gr.NONE)
    d.update(kw)
    return d


def test_three_works_in_two_overlapping_groups():
    # work 0 covers 0..5, work 1 covers 3..8 (inexact), work 2 has two records and no passage;
    # group 0 = {0, 1}, group 1 = {1, 2}, group 2 = nobody; scenes: words 0..4 -> 0, 5..9 -> 1
    recs = _diag(0, 0, 0, 6) + _diag(1, 0, 3, 6, exact=0) + [(2, 0, 9, 1), (2, 5, 0, 0)]
    label_of = [0] * 5 + [1] * 5
    found, cells, rows = gr.groups(recs, 3, 10, [[0], [0, 1], [1]], 3, label_of, 2)
    assert found == [
        _group(n_works=2, n_passage_works=2, n_words=12, n_exact=6, n_passages=2,
               passage_words=12, longest=6, covered=9, peak=2, peak_first=3, top_label=0,
               top_label_words=7, n_cells=2, n_word_rows=9),
        _group(n_works=2, n_passage_works=1, n_words=8, n_exact=1, n_passages=1, passage_words=6,
               longest=6, covered=6, peak=1, peak_first=3, top_label=1, top_label_words=5,
               n_cells=2, n_word_rows=6),
        _group()]
    assert cells == [dict(group=0, label=0, n_words=7, n_exact=5, n_works=2),
                     dict(group=0, label=1, n_words=5, n_exact=1, n_works=2),
                     dict(group=1, label=0, n_words=3, n_exact=0, n_works=2),
                     dict(group=1, label=1, n_words=5, n_exact=1, n_works=2)]
    assert [(r["group"], r["orig_ix"], r["n_works"]) for r in rows] == (
        [(0, o, 2 if 3 <= o <= 5 else 1) for o in range(9)] + [(1, o, 1) for o in range(3, 9)])
    found2, _, rows2 = gr.groups(recs, 3, 10, [[0], [0, 1], [1]], 3, label_of, 2, min_works=2)
    assert [(r["group"], r["orig_ix"]) for r in rows2] == [(0, 3), (0, 4), (0, 5)]
    assert [d["n_word_rows"] for d in found2] == [3, 0, 0] and found2[0]["covered"] == 9
    # a tie between the scenes goes to the first one; without labels no cells
    found3, cells3, _ = gr.groups(_diag(0, 0, 2, 6), 1, 10, [[0]], 1, label_of, 2)
    assert (found3[0]["top_label"], found3[0]["top_label_words"]) == (0, 3) and len(cells3) == 2
    found4, cells4, _ = gr.groups(_diag(0, 0, 2, 6), 1, 10, [[0]], 1)
    assert found4[0]["top_label"] == gr.NONE and cells4 == [] and found4[0]["covered"] == 6


def test_a_bridged_word_counts_in_depth_but_not_in_matched_words():
    recs = [(0, f, f, 1) for f in (0, 1, 2, 4, 5, 6)] + _diag(1, 0, 3, 6)
    found, _, rows = gr.groups(recs, 2, 9, [[0], [0]], 1, min_words=3, max_gap=1)
    assert (found[0]["n_words"], found[0]["covered"], found[0]["peak"]) == (12, 9, 2)
    assert [r["n_works"] for r in rows] == [1, 1, 1, 2, 2, 2, 2, 1, 1] and found[0]["peak_first"] == 3
    found, _, rows = gr.groups(recs, 2, 9, [[0], [0]], 1, min_words=3, max_gap=0)
    assert [r["n_works"] for r in rows] == [1, 1, 1, 1, 2, 2, 2, 1, 1]


def test_a_work_repeating_a_line_counts_once():
    recs = [r for k in range(10) for r in _diag(0, 20 * k, 10, 6)] + _diag(1, 0, 10, 6)
    found, _, rows = gr.groups(recs, 2, 16, [[0], [0]], 1)
    assert (found[0]["n_passages"], found[0]["passage_words"], found[0]["n_words"]) == (11, 66, 66)
    assert found[0]["peak"] == 2 and [r["n_works"] for r in rows] == [2] * 6


def test_oracle_refusals():
    ok = _diag(0, 0, 0, 3)
    for kw in (dict(min_words=0), dict(min_works=0), dict(n_works=2), dict(n_script=2),
               dict(n_groups=1), dict(members_of=[[1, 1]]), dict(members_of=[[1, 0]]),
               dict(label_of=[0, 0, 2], n_labels=2)):
        args = dict(n_works=1, n_script=3, members_of=[[0, 1]], n_groups=2, min_words=1)
        args.update(kw)
        with pytest.raises(ValueError):
            gr.groups(ok, **args)
    with pytest.raises(ValueError):
        gr.groups([(0, 1, 0, 1), (0, 0, 1, 1)], 1, 3, [[0]], 1)


def _row(name, fan, orig, scene="1", char="ANNA", comb="0.0"):
    return [name, fan, "f%d" % fan, 1, orig, "W%d" % orig, 2, char, scene, "0.0", 7, comb]


def _match_csv(rows):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


def test_the_three_files():
    rows = ([_row("b/123.txt", f, f + 10, scene="3", char="BOB") for f in (0, 1, 2, 4, 5, 6)] +
            [_row("125.txt", f, f + 14, scene="3", char="BOB", comb="0.5") for f in range(6)] +
            [_row("777.txt", f, f + 40) for f in range(6)] + [_row("124.txt", 0, 12, "3", "BOB")])
    g, s, w = gr.groups_csv(_match_csv(rows), _meta_text(ROWS), "year", 6, 1, 2)
    assert g.split("\r\n")[1:] == ["2016,1,1,1,6,6,1,6,6,7,1,10,3,6", "2019,1,0,0,0,0,0,0,0,0,0,,,0",
                                   "(unknown date),2,2,1,7,1,1,6,6,6,1,14,3,7",
                                   "(no metadata),0,1,1,6,6,1,6,6,6,1,40,1,6", ""]
    assert s.split("\r\n")[1:] == ["2016,3,6,6,1", "(unknown date),3,7,1,2", "(no metadata),1,6,6,1",
                                   ""]
    assert w == ",".join(gr.WORD_FIELDS) + "\r\n"            # no word of depth 2 in any group
    g, s, w = gr.groups_csv(_match_csv(rows), _meta_text(ROWS), "language", 6, 1, 1)
    assert [r.split(",")[0] for r in g.split("\r\n")[1:-1]] == ["(empty)", "Deutsch", "English",
                                                               "Italiano", "(no metadata)"]
    assert "English,13,[?],,,1" in w.split("\r\n")           # bridged: no record names it
    with pytest.raises(ValueError):
        gr.groups_csv(_match_csv(rows + [_row("x/123.html", 0, 1)]), _meta_text(ROWS))


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    args = cli.build_parser().parse_args(["groups", "runs/match-6gram-20240101.csv", "meta.csv"])
    assert args.func.__name__ == "_groups"
    assert (args.meta, args.by, args.output, args.min_words, args.max_gap, args.min_works,
            args.device, args.reader) == ("meta.csv", "year", None, 6, 0, 1, 0, None)
    assert groups.output_names(args.matches) == (
        "runs/match-6gram-20240101-groups.csv", "runs/match-6gram-20240101-groups-scenes.csv",
        "runs/match-6gram-20240101-groups-words.csv")
    assert groups.output_names("batch", None)[0] == "batch-groups.csv"
    assert groups.output_names("m.csv", "out/x")[2] == "out/x-groups-words.csv"
    args = cli.build_parser().parse_args(["groups", "m.csv", "meta.csv", "--by", "tag:Rating",
                                          "-o", "p", "--min-words", "3", "--max-gap", "2",
                                          "--min-works", "4", "--device", "1"])
    assert (args.by, args.output, args.min_words, args.max_gap, args.min_works, args.device) == \
        ("tag:Rating", "p", 3, 2, 4, 1)
    assert groups.GROUP_FIELDS == gr.GROUP_FIELDS and groups.SCENE_FIELDS == gr.SCENE_FIELDS
    assert groups.WORD_FIELDS == gr.WORD_FIELDS and groups.UNKNOWN_WORD == gr.UNKNOWN_WORD
    assert list(groups.LAST_GROUPS) == gr.LAST
    assert "groups" in cli.build_parser().format_help()


@pytest.mark.parametrize("bad", [["--min-works", "0"], ["--min-words", "0"], ["--max-gap", "-1"],
                                 ["--by", "decade"], ["--by", "tag:"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["groups", str(tmp_path / "none.csv"), str(tmp_path / "none-meta.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py groups: error: ")


def test_metadata_errors_exit_before_the_match_file_is_read(tmp_path):
    path = tmp_path / "meta.csv"
    for rows, by, what in ((ROWS + [dict(FILENAME="x/123.txt")], "year", "'123'"),
                           ([dict(ROWS[0], TAGS="[]")], "tag", "works/123.html")):
        path.write_text(_meta_text(rows), newline="", encoding="utf-8")
        with pytest.raises(SystemExit) as e:
            cli.main(["groups", str(tmp_path / "none.csv"), str(path), "--by", by])
        assert str(e.value.code).startswith("ao3.py groups: error: ") and what in str(e.value.code)


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_groups_entry_points():
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_groups", "fs_groups_rows", "fs_groups_times"):
        assert name in _declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("struct,dtype,size,keys",
                         [("fs_group", "GROUP_DTYPE", 64, gr.GROUP_KEYS + ["reserved", "reserved2"]),
                          ("fs_group_cell", "GROUP_CELL_DTYPE", 24, gr.CELL_KEYS + ["reserved"]),
                          ("fs_group_word", "GROUP_WORD_DTYPE", 16, gr.WORD_KEYS + ["reserved"])])
def test_dtypes_match_the_header(struct, dtype, size, keys):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for names in re.findall(r"uint32_t\s+([^;]+);", body):
        fields += [n.strip() for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == size == 4 * len(fields)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, 4 * k) for k, n in enumerate(fields)]
    assert list(dt.names) == keys
    assert re.search(r"#define FS_GROUPS_MAX_BYTES \(1u << 30\)", text)
    assert abi.FS_GROUPS_MAX_BYTES == 1 << 30


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = (C.c_uint64(7), C.c_uint64(7))
    z = np.zeros(4, dtype=np.uint32)
    out = np.ones(2, dtype=abi.GROUP_DTYPE)
    u32, u8 = abi.ptr(z, C.c_uint32), abi.ptr(z.view(np.uint8), C.c_uint8)
    off = np.array([0, 1, 2], dtype=np.uint64)

    def call(n_rows=1, n_script=4, min_words=6, min_works=1, groups=out.ctypes.data_as(C.c_void_p),
             cap=0, n_cells=C.byref(n[0]), off=off, n_groups=2, n_labels=0, grp=(0, 1)):
        g = np.array(grp, dtype=np.uint32)
        return L.fs_groups(0, u32, u32, u32, u8, n_rows, 2, n_script,
                           abi.ptr(np.asarray(off, dtype=np.uint64), C.c_uint64),
                           abi.ptr(g, C.c_uint32), n_groups, u32 if n_labels else None, n_labels,
                           min_words, 0, min_works, groups, None, cap, n_cells, None, 0,
                           C.byref(n[1]))
    assert call(min_words=0) == abi.FS_E_INVALID
    assert call(min_works=0) == abi.FS_E_INVALID
    assert b"at least 1" in L.fs_last_error()
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(groups=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                     # a capacity without a buffer
    assert call(n_cells=None) == abi.FS_E_INVALID
    assert call(off=[1, 1, 2]) == abi.FS_E_INVALID             # mem_off[0] != 0
    assert call(off=[0, 2, 1]) == abi.FS_E_INVALID             # mem_off decreases
    assert call(n_groups=1) == abi.FS_E_INVALID                # a group >= n_groups
    assert call(off=[0, 2, 2], grp=(1, 1)) == abi.FS_E_INVALID   # not strictly ascending
    # tables above the cap: refused from the sizes alone, nothing allocated, no device touched
    assert call(n_groups=21846, n_labels=4096) == abi.FS_E_UNSUPPORTED
    assert b"more than" in L.fs_last_error()
    # no records: groups without counts, without device work
    assert call(n_rows=0) == abi.FS_OK and (n[0].value, n[1].value) == (0, 0)
    assert out.tolist() == [(0,) * 9 + (gr.NONE, gr.NONE) + (0,) * 5] * 2
    assert L.fs_groups_rows(None, None, 0, 0, None, None, 0, None, 0, 6, 0, 1, None, None, 0,
                            C.byref(n[0]), None, 0, C.byref(n[1])) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_cases_are_those_of_the_issue():
    from tests.golden import make_quotes_golden as mqg
    assert {c[4] for c in mgg.CASES} == {"year", "tag", "tag:Relationship"}
    assert {c[:4] for c in mgg.CASES} == {c[:4] for c in mqg.CASES} and len(mgg.CASES) == 21
    with open(os.path.join(GOLDEN, mgg.META), newline="", encoding="utf-8") as fh:
        rows = list(csv.DictReader(fh))
    assert list(rows[0]) == groups.META_FIELDS
    stems = {gr.stem(r["FILENAME"]) for r in rows}
    assert "never_searched" in stems and "d" not in stems and "w0000006" not in stems


@pytest.mark.parametrize("case,src,m,g,by", mgg.CASES)
def test_golden_files_are_the_oracle_output(case, src, m, g, by):
    with open(os.path.join(GOLDEN, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    with open(os.path.join(GOLDEN, mgg.META), newline="", encoding="utf-8") as fh:
        meta = fh.read()
    got = gr.groups_csv(text, meta, by, m, g, 1)
    for name, part in zip(mgg.golden_names(case, m, g, by), got):
        with open(os.path.join(GOLDEN, name), newline="", encoding="utf-8") as fh:
            want = fh.read()
        assert part == want, name
        assert want.count("\r\n") > 1                   # no file is empty
    assert ("(no metadata)" in got[0]) == (case in ("matrix_spans_a", "synthetic_small"))
