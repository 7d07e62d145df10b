"""`ao3.py variants` without a GPU: the oracle's known answers (tests/variants_restated.py), the
parser, the C ABI's declarations and the committed expected CSVs."""

import csv
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from fandom_search_amd import _lib, abi, cli
from tests import passages_restated as pr
from tests import variants_restated as vr
from tests.golden import make_variants_golden as mvg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cell(orig_ix, spell, n_records, n_works):
    return dict(orig_ix=orig_ix, spell=spell, n_records=n_records, n_works=n_works)


def _word(n_records=0, n_spellings=0, n_works=0, first_cell=vr.NONE):
    return dict(n_records=n_records, n_spellings=n_spellings, n_works=n_works,
                first_cell=first_cell)


# ---- oracle known answers -------------------------------------------------------------

def test_interning_numbers_spellings_in_first_appearance_order():
    ids, first = vr.intern([b"b", b"a", b"b", b'"a"', b"", b"a", b""])
    assert ids == [0, 1, 0, 2, 3, 1, 3] and first == [0, 1, 3, 4]
    assert vr.intern([]) == ([], [])


def test_cells_and_words_of_hand_written_records():
    recs = [(0, 5, 2), (1, 5, 2), (1, 5, 0), (0, 7, 1), (0, 5, 2), (2, 7, 1), (2, 5, 0)]
    words, cells = vr.variants(recs, 3, 9, 3)
    assert cells == [_cell(5, 2, 3, 2), _cell(5, 0, 2, 2), _cell(7, 1, 2, 2)]
    assert words[5] == _word(5, 2, 3, 0) and words[7] == _word(2, 1, 2, 2)
    assert words[0] == words[6] == words[8] == _word()
    # the order of the records does not matter
    assert vr.variants(recs[::-1], 3, 9, 3) == (words, cells)


def test_the_tie_rules():
    # equal records: more works first; equal in both: the smaller spelling id first
    recs = [(0, 1, 3), (0, 1, 3), (0, 1, 2), (1, 1, 2), (0, 1, 1), (1, 1, 1), (0, 1, 0)]
    _, cells = vr.variants(recs, 2, 2, 4)
    assert [(c["spell"], c["n_records"], c["n_works"]) for c in cells] == \
        [(1, 2, 2), (2, 2, 2), (3, 2, 1), (0, 1, 1)]


def test_refusals_and_no_records():
    for bad in ((2, 0, 0), (0, 3, 0), (0, 0, 4)):
        with pytest.raises(ValueError):
            vr.variants([(0, 0, 0), bad], 2, 3, 4)
    with pytest.raises(NotImplementedError):
        vr.variants([], 1, (1 << 19) + 1, 1)
    assert vr.variants([], 0, 2, 0) == ([_word(), _word()], [])


def _row(name, fan, fan_word, orig, word, char="ANNA", scene="1"):
    return [name, fan, fan_word, 1, orig, word, 2, char, scene, "0.0", 7, "0.0"]


def _match_csv(rows, header=True):
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    if header:
        w.writerow(pr.MATCH_FIELDS)
    w.writerows(rows)
    return buf.getvalue()


ROWS = [_row("a.txt", 0, "Luke", 4, "luke"), _row("a.txt", 1, "luke", 4, "luke"),
        _row("b.txt", 0, "LUKE", 4, "luke"), _row("b.txt", 1, "Luke", 4, "luke"),
        _row("b.txt", 2, "dad", 6, "father"), _row("a.txt", 9, "dad", 6, "father")]


def test_the_two_files():
    cells, words = vr.variants_csv(_match_csv(ROWS))
    assert cells.split("\r\n")[1:] == [
        "4,luke,ANNA,1,1,Luke,2,2,0", "4,luke,ANNA,1,2,luke,1,1,1", "4,luke,ANNA,1,3,LUKE,1,1,0",
        "6,father,ANNA,1,1,dad,2,2,0", ""]
    assert words.split("\r\n")[1:] == ["4,luke,ANNA,1,4,2,3,1,Luke,2",
                                       "6,father,ANNA,1,2,2,1,0,dad,2", ""]
    assert vr.variants_csv(_match_csv(ROWS, header=False)) == (cells, words)


def test_fold_case_merges_and_shows_the_first_appearance():
    cells, words = vr.variants_csv(_match_csv(ROWS), fold_case=True)
    assert cells.split("\r\n")[1:3] == ["4,luke,ANNA,1,1,Luke,4,2,1", "6,father,ANNA,1,1,dad,2,2,0"]
    assert words.split("\r\n")[1] == "4,luke,ANNA,1,4,2,1,4,Luke,4"


def test_top_and_min_records_leave_the_words_file_alone():
    base = vr.variants_csv(_match_csv(ROWS), top=0)
    cut = vr.variants_csv(_match_csv(ROWS), top=1, min_records=2)
    assert cut[1] == base[1]
    assert cut[0].split("\r\n")[1:] == ["4,luke,ANNA,1,1,Luke,2,2,0",
                                        "6,father,ANNA,1,1,dad,2,2,0", ""]
    # a rank is the spelling's place among all spellings of the word
    assert vr.variants_csv(_match_csv(ROWS[:4] + [ROWS[1]] * 2), min_records=2)[0].split("\r\n")[1:3] \
        == ["4,luke,ANNA,1,1,luke,3,1,1", "4,luke,ANNA,1,2,Luke,2,2,0"]


def test_a_script_word_with_two_labels_is_an_error():
    rows = ROWS + [_row("c.txt", 0, "x", 4, "luke", scene="9")]
    with pytest.raises(ValueError):
        vr.variants_csv(_match_csv(rows))


def test_empty_input():
    cells, words = vr.variants_csv("")
    assert cells == ",".join(vr.CELL_FIELDS) + "\r\n"
    assert words == ",".join(vr.WORD_FIELDS) + "\r\n"


# ---- product side that needs no GPU ----------------------------------------------------

def test_parser_defaults_and_output_names():
    from fandom_search_amd import variants
    args = cli.build_parser().parse_args(["variants", "runs/match-6gram-20240101.csv"])
    assert args.func.__name__ == "_variants"
    assert (args.output, args.top, args.min_records, args.fold_case, args.device, args.reader) == \
        (None, 10, 1, False, 0, None)
    assert variants.output_names(args.matches) == ("runs/match-6gram-20240101-variants.csv",
                                                   "runs/match-6gram-20240101-variants-words.csv")
    assert variants.output_names("batch", None)[0] == "batch-variants.csv"
    assert variants.output_names("m.csv", "out/x")[1] == "out/x-variants-words.csv"
    args = cli.build_parser().parse_args(["variants", "m.csv", "-o", "p", "--top", "0",
                                          "--min-records", "3", "--fold-case", "--device", "1",
                                          "--reader", "python"])
    assert (args.output, args.top, args.min_records, args.fold_case, args.device, args.reader) == \
        ("p", 0, 3, True, 1, "python")
    assert variants.CELL_FIELDS == vr.CELL_FIELDS and variants.WORD_FIELDS == vr.WORD_FIELDS


@pytest.mark.parametrize("bad", [["--top", "-1"], ["--min-records", "0"]])
def test_bad_arguments_exit_with_an_error_line(bad, tmp_path):
    with pytest.raises(SystemExit) as e:
        cli.main(["variants", str(tmp_path / "none.csv")] + bad)
    assert str(e.value.code).startswith("ao3.py variants: error: ")


def test_merge_spellings():
    from fandom_search_amd import variants
    remap, ids, shown = variants.merge_spellings(["Luke", "luke", "Luke", "", "LUKE"])
    assert remap.tolist() == [0, 1, 0, 2, 3] and shown == ["Luke", "luke", "", "LUKE"]
    remap, ids, shown = variants.merge_spellings(["Luke", "luke", "Luke", "", "LUKE"], True)
    assert remap.tolist() == [0, 0, 0, 1, 0] and shown == ["Luke", ""] and ids == {"luke": 0, "": 1}


def test_abi_declares_and_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    declared = set(re.findall(r"\b(fs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    if not os.path.exists(_lib.lib_path()):
        _lib.build()
    lib = C.CDLL(_lib.lib_path())
    for name in ("fs_variants", "fs_matches_intern", "fs_matches_intern_times"):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name)


@pytest.mark.parametrize("struct,dtype,keys", [("fs_variant_cell", "VARIANT_CELL_DTYPE", vr.CELL_KEYS),
                                               ("fs_variant_word", "VARIANT_WORD_DTYPE", vr.WORD_KEYS)])
def test_dtypes_match_the_header(struct, dtype, keys):
    text = open(os.path.join(ROOT, "include", "fandom_search.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for names in re.findall(r"uint32_t\s+([^;]+);", body):
        fields += [n.strip() for n in names.split(",")]
    dt = getattr(abi, dtype)
    assert dt.itemsize == 16 == 4 * len(fields)
    assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, 4 * k) for k, n in enumerate(fields)]
    assert list(dt.names) == keys


def test_argument_rules_that_need_no_device():
    L = _lib.load()
    n = C.c_uint64(7)
    z = np.zeros(4, dtype=np.uint32)
    words = np.ones(4, dtype=abi.VARIANT_WORD_DTYPE)
    u32 = abi.ptr(z, C.c_uint32)
    w = words.ctypes.data_as(C.c_void_p)

    def call(n_rows=1, n_script=4, words=w, cap=0, n_cells=C.byref(n)):
        return L.fs_variants(0, u32, u32, u32, n_rows, 2, n_script, 2, words, None, cap, n_cells)
    assert call(n_rows=1 << 32) == abi.FS_E_UNSUPPORTED
    assert call(n_script=(1 << 19) + 1) == abi.FS_E_UNSUPPORTED
    assert call(words=None) == abi.FS_E_INVALID
    assert call(cap=1) == abi.FS_E_INVALID                     # a capacity without a buffer
    assert call(n_cells=None) == abi.FS_E_INVALID
    # no records: empty words without device work
    assert call(n_rows=0) == abi.FS_OK and n.value == 0
    assert (words["first_cell"] == vr.NONE).all()
    assert not any(words[name].any() for name in vr.WORD_KEYS[:-1])
    assert L.fs_matches_intern(None, 2, None, None, 0, C.byref(n)) == abi.FS_E_INVALID
    assert L.fs_matches_intern_times(None, None) == abi.FS_E_INVALID


# ---- committed expected outputs ---------------------------------------------------------

def test_the_golden_generator_reproduces_its_committed_files():
    made = mvg.build()
    assert set(made) == {mvg.INPUT} | {n for c in mvg.CASES for n in mvg.golden_names(c[0])}
    for name, text in made.items():
        with open(os.path.join(GOLDEN, name), "rb") as fh:
            assert fh.read() == text.encode("utf-8"), name


def test_the_golden_input_holds_what_the_issue_asks_for():
    rows = pr.read_rows(mvg.input_csv())
    assert 200 <= len(rows) <= 400
    spellings = {}
    for r in rows:
        spellings.setdefault(int(r[4]), set()).add(r[2])
    counts = sorted(len(s) for s in spellings.values())
    assert counts[0] == 1 and 2 in counts and 65 < counts[-1] < 80
    fans = {r[2] for r in rows}
    assert {"Luke", "luke", "LUKE", ""} <= fans
    assert any("," in f for f in fans) and any('"' in f for f in fans)
    assert any(not f.isascii() for f in fans)
    names = [r[0] for r in rows]
    blocks = [n for k, n in enumerate(names) if k == 0 or names[k - 1] != n]
    assert len(blocks) > len(set(blocks))                      # a work comes back
    cells = vr.variants_csv(mvg.input_csv(), top=0)[0].split("\r\n")
    assert "13,feeling,HAN,4,1,sense,2,2,0" in cells and "13,feeling,HAN,4,2,feelin,2,1,0" in cells
    assert cells.index("14,bad,HAN,4,2,terrible,1,1,0") + 1 == cells.index("14,bad,HAN,4,3,awful,1,1,0")
