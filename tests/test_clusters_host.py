"""`ao3.py clusters` without a GPU: the oracle's known answers, the parser, the C ABI's
declarations and the committed expected CSVs."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import clusters_restated as cr
from tests import pairs_restated as pp
from tests.golden import make_clusters_golden as mcg
from tests.golden import make_pairs_golden as mpg
from tests.test_pairs_host import _match_csv, _row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = cr.NONE


def spans(spans_of):
    """Records of works given as lists of (first script word, words), one diagonal run each."""
    recs = []
    for w, sp in enumerate(spans_of):
        f = 0
        for o0, k in sp:
            recs += [(w, f + i, o0 + i) for i in range(k)]
            f += k + 10
    return recs


def run(spans_of, n_script=200, **kw):
    args = dict(min_words=1, min_shared=1, min_jaccard=0, min_size=2, common_pct=50)
    args.update(kw)
    return cr.clusters(spans(spans_of), len(spans_of), n_script, **args)


# ---- oracle known answers -------------------------------------------------------------

def test_a_chain_is_one_family_although_its_ends_share_nothing():
    works, found = run([[(0, 10)], [(8, 10)], [(16, 10)]])
    assert [(w["root"], w["size"], w["cluster"], w["links"]) for w in works] == \
        [(0, 3, 0, 1), (0, 3, 0, 2), (0, 3, 0, 1)]
    assert found == [dict(root=0, n_works=3, n_links=2, hub=1, hub_links=2, covered=26,
                          common=4, peak=2, peak_first=8, run_first=8, run_words=2)]
    assert works[0]["best"] == 1 and works[2]["best"] == 1 and works[1]["best"] == 0


def test_the_root_is_the_smallest_work_whatever_the_order_of_the_links():
    # the links are (3, 4), (2, 3), (1, 2), (0, 1) when met from the last work down; work 5
    # shares with nobody
    works, found = run([[(0, 10)], [(8, 10)], [(16, 10)], [(24, 10)], [(32, 10)], [(100, 4)]])
    assert [w["root"] for w in works] == [0, 0, 0, 0, 0, 5]
    assert [w["size"] for w in works] == [5, 5, 5, 5, 5, 1]
    assert len(found) == 1 and found[0]["root"] == 0 and found[0]["n_links"] == 4
    # an inactive work between: no root, no size, no family
    works, found = run([[], [(0, 10)], [], [(5, 10)]])
    assert [(w["root"], w["size"], w["cluster"]) for w in works] == \
        [(NONE, 0, NONE), (1, 2, 0), (NONE, 0, NONE), (1, 2, 0)]


def test_a_jaccard_at_the_threshold_links_and_one_word_less_does_not():
    # 10 and 10 words sharing 5: union 15, 100 * 5 / 15 = 33.3; sharing 4 of 8 and 8: 4 / 12
    a, b = [(0, 8)], [(4, 8)]
    for j, want in ((33, 1), (34, 0)):
        works, found = run([a, b], min_jaccard=j)
        assert len(found) == want
    # exactly at it: 5 shared of a union of 10 is 50 per cent
    works, found = run([[(0, 10)], [(5, 5)]], min_jaccard=50)
    assert len(found) == 1 and works[0]["best_shared"] == 5
    works, found = run([[(0, 10)], [(6, 4)]], min_jaccard=50)       # 4 of 10
    assert found == [] and works[0]["links"] == 0 and works[0]["best"] == NONE
    works, found = run([[(0, 10)], [(6, 5)]], min_jaccard=50)       # 4 of 11
    assert found == []
    assert cr.linked(set(range(10)), set(range(5, 10)), 1, 50) == (True, 5)
    assert cr.linked(set(range(10)), set(range(5, 10)), 6, 0) == (False, 5)
    # identical works are linked at 100, and only they
    works, found = run([[(0, 6)], [(0, 6)], [(0, 7)]], min_jaccard=100)
    assert [w["root"] for w in works] == [0, 0, 2]


def test_min_jaccard_0_gives_the_components_of_the_kept_pairs():
    rng = np.random.default_rng(5)
    spans_of = [[(int(rng.integers(0, 180)), int(rng.integers(3, 12)))
                 for _ in range(int(rng.integers(0, 3)))] for _ in range(40)]
    recs = spans(spans_of)
    works, found = cr.clusters(recs, 40, 200, 3, 0, 4, 0, 1, 50)
    pw, pairs = pp.pairs(recs, 40, 200, 3, 0, 4)
    comp = {w: {w} for w in range(40) if pw[w]["covered"]}
    for p in pairs:
        merged = comp[p["a"]] | comp[p["b"]]
        for w in merged:
            comp[w] = merged
    assert len(pairs) > 5
    for w in range(40):
        assert works[w]["covered"] == pw[w]["covered"]
        assert works[w]["links"] == pw[w]["partners"]
        assert (works[w]["best"], works[w]["best_shared"]) == (pw[w]["best"], pw[w]["best_shared"])
        assert works[w]["root"] == (min(comp[w]) if w in comp else NONE)
        assert works[w]["size"] == (len(comp[w]) if w in comp else 0)
    assert sum(c["n_links"] for c in found) == len(pairs)
    assert [c["root"] for c in found] == sorted({min(s) for s in comp.values()})


def test_min_size_1_lists_single_works():
    spans_of = [[(0, 6)], [(50, 6)], [(0, 6)], []]
    works, found = run(spans_of, min_size=1)
    assert [(c["root"], c["n_works"], c["n_links"], c["hub"], c["hub_links"]) for c in found] == \
        [(0, 2, 1, 0, 1), (1, 1, 0, 1, 0)]
    assert [w["cluster"] for w in works] == [0, 1, 0, NONE]
    works, found = run(spans_of, min_size=2)
    assert [c["root"] for c in found] == [0] and [w["cluster"] for w in works] == [0, NONE, 0, NONE]
    assert (works[1]["root"], works[1]["size"]) == (1, 1)
    assert run(spans_of, min_size=3)[1] == []


def test_the_hub_tie_goes_to_the_smaller_work():
    # a ring of four: every work has two links
    works, found = run([[(0, 10), (38, 2)], [(8, 12)], [(18, 12)], [(28, 12)]])
    assert [w["links"] for w in works] == [2, 2, 2, 2]
    assert (found[0]["hub"], found[0]["hub_links"], found[0]["n_links"]) == (0, 2, 4)
    # works 2 and 3 have the most links, two each
    works, found = run([[(0, 5)], [(20, 5)], [(3, 10)], [(12, 10)], [(40, 5)]])
    assert [w["links"] for w in works] == [1, 1, 2, 2, 0]
    assert (found[0]["hub"], found[0]["hub_links"]) == (2, 2)


def test_the_common_run_is_the_first_among_equals_and_crosses_a_word_boundary():
    # two works: common (both, at 100 per cent) are 10..12, 20..22 and 60..67
    works, found = run([[(10, 3), (20, 3), (60, 8)], [(0, 100)]], common_pct=100)
    assert (found[0]["common"], found[0]["run_first"], found[0]["run_words"]) == (14, 60, 8)
    works, found = run([[(10, 3), (20, 3)], [(0, 100)]], common_pct=100)
    assert (found[0]["common"], found[0]["run_first"], found[0]["run_words"]) == (6, 10, 3)
    assert (found[0]["peak"], found[0]["peak_first"], found[0]["covered"]) == (2, 10, 100)
    # at 50 per cent of two works one is enough: t = 1
    works, found = run([[(10, 3), (20, 3)], [(30, 40), (10, 1)]], common_pct=50)
    assert (found[0]["common"], found[0]["run_first"], found[0]["run_words"]) == (46, 30, 40)
    # t = (common_pct * n_works + 99) / 100: of three works, 34 per cent asks for two
    three = [[(0, 10)], [(5, 10)], [(12, 10)]]
    assert run(three, common_pct=33)[1][0]["common"] == 22
    assert run(three, common_pct=34)[1][0]["common"] == 8


def test_common_is_0_at_100_per_cent_on_a_chain():
    works, found = run([[(0, 10)], [(8, 10)], [(16, 10)]], common_pct=100)
    assert (found[0]["common"], found[0]["run_first"], found[0]["run_words"]) == (0, NONE, 0)
    assert (found[0]["covered"], found[0]["peak"], found[0]["peak_first"]) == (26, 2, 8)


def test_a_work_repeating_a_line_counts_it_once():
    works, found = run([[(10, 6), (10, 6)], [(10, 6)]], min_jaccard=100)
    assert works[0]["covered"] == 6 and works[0]["best_shared"] == 6
    assert found == [dict(root=0, n_works=2, n_links=1, hub=0, hub_links=1, covered=6, common=6,
                          peak=2, peak_first=10, run_first=10, run_words=6)]


def test_refusals_and_no_records():
    ok = [(0, 0, 0), (0, 1, 1)]
    for kw in (dict(min_words=0), dict(min_shared=0), dict(min_size=0), dict(common_pct=0),
               dict(common_pct=101), dict(min_jaccard=101), dict(n_works=0), dict(n_script=1)):
        args = dict(n_works=1, n_script=2, min_words=1)
        args.update(kw)
        with pytest.raises(ValueError):
            cr.clusters(ok, **args)
    with pytest.raises(ValueError):
        cr.clusters([(0, 1, 0), (0, 0, 1)], 1, 3)
    none = dict(covered=0, root=NONE, size=0, cluster=NONE, links=0, best=NONE, best_shared=0)
    assert cr.clusters([], 2, 2) == ([none, none], [])


def test_the_two_files():
    rows = ([_row("b.txt", f, f + 10, scene="3", char="BOB") for f in (0, 1, 2, 4, 5, 6)] +
            [_row("a.txt", f, f + 11, scene="3", char="BOB") for f in (0, 1, 3, 4, 5, 6)] +
            [_row("c.txt", f, f + 40) for f in range(6)] + [_row("d.txt", 0, 12, "3", "BOB")] +
            [_row("e.txt", f, f + 40) for f in range(7)] +
            [_row("f.txt", f, f + 41) for f in range(6)])
    found, works = cr.clusters_csv(_match_csv(rows), 6, 1, 1, 50, 2, 100)
    # c, e and f: 40..45, 40..46, 41..46, every pair linked; b covers 10..16, a 11..17, both
    # bridge word 13, which no record names.  The larger family comes first.
    assert found.split("\r\n")[1:] == [
        "1,3,3,c.txt,2,7,5,3,41,41,5,ANNA,1,W41 W42 W43 W44 W45",
        "2,2,1,b.txt,1,8,6,2,11,11,6,BOB,3,W11 W12 [?] W14 W15 W16", ""]
    assert works.split("\r\n")[1:] == [
        "b.txt,2,2,7,1,a.txt,6", "a.txt,2,2,7,1,b.txt,6", "c.txt,1,3,6,2,e.txt,6",
        "e.txt,1,3,7,2,c.txt,6", "f.txt,1,3,6,2,e.txt,6", ""]
    assert cr.clusters_csv(_match_csv(rows, header=False), 6, 1, 1, 50, 2, 100) == (found, works)
    # no common word: a start, a character, a scene and a text there are not
    rows = ([_row("a.txt", f, f) for f in range(10)] + [_row("b.txt", f, f + 8) for f in range(10)] +
            [_row("c.txt", f, f + 16) for f in range(10)])
    found, works = cr.clusters_csv(_match_csv(rows), 6, 0, 1, 0, 2, 100)
    assert found.split("\r\n")[1:] == ["1,3,2,b.txt,2,26,0,2,8,,0,,,", ""]
    empty = cr.clusters_csv("")
    assert empty == (",".join(cr.CLUSTER_FIELDS) + "\r\n", ",".join(cr.WORK_FIELDS) + "\r\n")


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import clusters
    args = cli.build_parser().parse_args(["clusters", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_clusters"
    assert (args.output, args.min_words, args.max_gap, args.min_shared, args.min_jaccard,
            args.min_size, args.common, args.device, args.reader) == \
        (None, 6, 0, 6, 50, 2, 50, 0, None)
    assert clusters.output_names(args.matches) == (
        "runs/match-6gram-20240101-clusters.csv", "runs/match-6gram-20240101-clusters-works.csv")
    assert clusters.output_names("batch", None)[0] == "batch-clusters.csv"
    assert clusters.output_names("m.csv", "out/x")[1] == "out/x-clusters-works.csv"
    args = cli.build_parser().parse_args(
        ["clusters", "m.csv", "-o", "p", "--min-words", "3", "--max-gap", "2", "--min-shared",
         "4", "--min-jaccard", "0", "--min-size", "1", "--common", "100", "--device", "1",
         "--reader", "python"])
    assert (args.output, args.min_words, args.max_gap, args.min_shared, args.min_jaccard,
            args.min_size, args.common, args.device, args.reader) == \
        ("p", 3, 2, 4, 0, 1, 100, 1, "python")
    assert clusters.CLUSTER_FIELDS == cr.CLUSTER_FIELDS
    assert clusters.WORK_FIELDS == cr.WORK_FIELDS
    assert clusters.UNKNOWN_WORD == cr.UNKNOWN_WORD == "[?]"
    assert "clusters" in cli.build_parser().format_help()


@pytest.mark.parametrize("bad", [["--min-shared", "0"], ["--min-words", "0"], ["--max-gap", "-1"],
                                 ["--min-size", "0"], ["--min-jaccard", "101"],
                                 ["--min-jaccard", "-1"], ["--common", "0"], ["--common", "101"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["clusters", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py clusters: error: ")


def test_a_script_word_with_two_labels_is_an_error(tmp_path):
    rows = [_row("a.txt", 0, 5), _row("a.txt", 1, 6), _row("b.txt", 0, 5, scene="4")]
    with pytest.raises(ValueError):
        cr.clusters_csv(_match_csv(rows))
    path = tmp_path / "two.csv"
    path.write_text(_match_csv(rows), newline="")
    with pytest.raises(SystemExit) as e:                  # (the labels are read before the GPU)
        cli.main(["clusters", str(path), "--reader", "python"])
    assert str(e.value.code).startswith("ao3.py clusters: error: script word 5 ")


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", text))


def test_abi_declares_and_exports_the_clusters_entry_points():
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_clusters", "fs_clusters_rows", "fs_clusters_times"):
        assert name in _declared_functions()
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)


@pytest.mark.parametrize("struct,dtype,size,keys",
                         [("fs_cluster_work", "CLUSTER_WORK_DTYPE", 32, cr.WORK_KEYS),
                          ("fs_cluster", "CLUSTER_DTYPE", 48, cr.CLUSTER_KEYS)])
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
    assert list(dt.names) == keys + ["reserved"]
    assert re.search(r"#define FS_CLUSTERS_MAX_BYTES \(1u << 30\)", text)
    assert abi.FS_CLUSTERS_MAX_BYTES == 1 << 30


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    works = np.ones(2, dtype=abi.CLUSTER_WORK_DTYPE)
    u32 = abi.ptr(z, C.c_uint32)
    w = works.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, min_words=6, min_shared=6, min_jaccard=50, min_size=2,
             common_pct=50, works=w, cap=0, n_clusters=C.byref(n)):
        return L.fs_clusters(0, u32, u32, u32, n_rows, 2, n_script, min_words, 0, min_shared,
                             min_jaccard, min_size, common_pct, works, None, cap, n_clusters)
    for zero in ("min_words", "min_shared", "min_size", "common_pct"):
        assert call(**{zero: 0}) == abi.FS_E_INVALID, zero
        assert b"at least 1" in L.fs_last_error()
    assert call(min_jaccard=101) == abi.FS_E_INVALID
    assert call(common_pct=101) == abi.FS_E_INVALID
    assert b"at most 100" in L.fs_last_error()
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(works=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                     # a capacity without a buffer
    assert call(n_clusters=None) == abi.FS_E_INVALID
    # no records: works without coverage, without device work
    assert call(n_rows=0, min_jaccard=0, common_pct=100) == abi.FS_OK and n.value == 0
    assert works.tolist() == [(0, NONE, 0, NONE, 0, NONE, 0, 0)] * 2
    assert L.fs_clusters_rows(None, None, 0, 0, 6, 0, 6, 50, 2, 50, None, None, 0,
                              C.byref(n)) == abi.FS_E_INVALID
    assert L.fs_clusters_times(None) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_cases_are_those_of_the_pairs_inputs():
    assert {c[:4] for c in mcg.CASES} == {c[:4] for c in mpg.CASES}
    assert len(mcg.CASES) == 14 and {c[4:] for c in mcg.CASES} == set(mcg.SETTINGS)


@pytest.mark.parametrize("case,src,m,g,s,j,z,p", mcg.CASES)
def test_golden_files_are_the_oracle_output(case, src, m, g, s, j, z, p):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, src), newline="", encoding="utf-8") as fh:
        text = fh.read()
    got = cr.clusters_csv(text, m, g, s, j, z, p)
    for name, part in zip(mcg.golden_names(case, m, g, s, j, z, p), got):
        with open(os.path.join(gold, name), newline="", encoding="utf-8") as fh:
            assert part == fh.read(), name
    assert got[1].count("\r\n") > 1                     # every case has active works


def test_a_golden_case_has_two_listed_families_and_an_unlisted_work():
    gold = os.path.join(ROOT, "tests", "golden")
    names = mcg.golden_names("synthetic_small", 6, 0, 1, 0, 2, 100)
    assert any(c[0] == "synthetic_small" and c[2:] == (6, 0, 1, 0, 2, 100) for c in mcg.CASES)
    with open(os.path.join(gold, names[0]), newline="", encoding="utf-8") as fh:
        assert fh.read().count("\r\n") - 1 >= 2
    with open(os.path.join(gold, names[1]), newline="", encoding="utf-8") as fh:
        rows = [line.split(",") for line in fh.read().split("\r\n")[1:-1]]
    assert sum(1 for r in rows if r[1] == "") >= 1 and sum(1 for r in rows if r[1] != "") >= 4
