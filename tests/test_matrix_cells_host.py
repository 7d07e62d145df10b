"""`ao3.py matrix --cells` and `--engine python` without a GPU: the cells file holds exactly the
non-zeros of the dense file written beside it, the dense file is the committed fixture byte for
byte, and the new reference-pinned fixtures of tests/golden/matrix_engine hold matrix.py."""

import csv
import glob
import os
import re
import sys

import pytest

from fandom_search_amd import matrix
from fandom_search_amd.cli import main
from tests import util

ENGINE = os.path.join(util.GOLDEN, "matrix_engine")
CASES = sorted(
    [(util.GOLDEN, "matrix_%s" % m.group(1), int(m.group(2)))
     for m in (re.match(r"matrix_(.+)\.n(\d+)\.csv$", os.path.basename(p))
               for p in glob.glob(os.path.join(util.GOLDEN, "matrix_*.n*.csv")))] +
    [(ENGINE, m.group(1), int(m.group(2)))
     for m in (re.match(r"(.+)\.n(\d+)\.csv$", os.path.basename(p))
               for p in glob.glob(os.path.join(ENGINE, "*.n*.csv")))])
IDS = ["%s.n%d" % (name, n) for _, name, n in CASES]


def read(path):
    with open(path, newline="") as fh:
        return fh.read()


def non_zeros(dense_path):
    """What the cells file must hold, from the dense file alone."""
    with open(dense_path, newline="") as fh:
        rows = list(csv.reader(fh))
    return [(row[0], k, rows[0][k], c) for row in rows[1:] for k, c in enumerate(row)
            if k and c != "0"]


def check_cells(cells_path, dense_path, src, n):
    with open(cells_path, newline="") as fh:
        cells = list(csv.reader(fh))
    assert cells[0] == ['FILENAME', 'PHRASE_INDEX', 'ORIGINAL_SCRIPT_WORD_INDEX', 'PHRASE',
                        'COUNT']
    assert [(r[0], int(r[1]), r[3], r[4]) for r in cells[1:]] == non_zeros(dense_path)
    # the start of a column: where the last kept n-gram that spells the phrase begins
    dd = matrix.StrictNgramDedupe(src, n)
    want = {}
    for m in dd.filtered_matches:
        want[dd.match_to_phrase(m)] = m[0]['ORIGINAL_SCRIPT_WORD_INDEX']
    assert all(r[2] == want[r[3]] for r in cells[1:])
    starts = [int(r[2]) for r in cells[1:] if r[0] == '(total)']
    assert starts == sorted(starts)


def test_fixtures_exist():
    assert len(CASES) >= 12 and sum(d == ENGINE for d, _, _ in CASES) >= 5


@pytest.mark.parametrize("where,name,n", CASES, ids=IDS)
def test_cells_are_the_non_zeros_of_the_dense_file(where, name, n, tmp_path):
    src = os.path.join(where, name + ".in.csv")
    prefix = str(tmp_path / "m")
    assert main(["matrix", src, prefix, "-n", str(n), "--cells", "--engine", "python"]) == 0
    dense = matrix.matrix_filename(prefix, n)
    assert read(dense) == read(os.path.join(where, "%s.n%d.csv" % (name, n)))
    check_cells(matrix.cells_filename(prefix, n), dense, src, n)
    assert sorted(os.listdir(tmp_path)) == sorted(
        os.path.basename(p) for p in (dense, matrix.cells_filename(prefix, n)))


@pytest.mark.parametrize("where,name,n", CASES, ids=IDS)
def test_no_cells_file_without_the_flag(where, name, n, tmp_path):
    src = os.path.join(where, name + ".in.csv")
    prefix = str(tmp_path / "m")
    loaded = set(sys.modules)
    assert main(["matrix", src, prefix, "-n", str(n), "--engine", "python"]) == 0
    assert os.listdir(tmp_path) == [os.path.basename(matrix.matrix_filename(prefix, n))]
    assert read(matrix.matrix_filename(prefix, n)) == \
        read(os.path.join(where, "%s.n%d.csv" % (name, n)))
    # the python engine needs neither the library nor the device reader
    assert not {"fandom_search_amd.matches"} & (set(sys.modules) - loaded)


def test_engine_fixtures_are_what_the_generator_writes():
    from tests.golden import make_matrix_engine_golden as mk
    seen = 0
    for name, n, text in mk.inputs():
        assert read(os.path.join(ENGINE, "%s.in.csv" % name)) == text
        assert (ENGINE, name, n) in CASES
        seen += 1
    assert seen == sum(d == ENGINE for d, _, _ in CASES)


def test_cells_of_an_empty_matrix(tmp_path):
    from tests.golden.make_matrix_golden import span_csv
    src = tmp_path / "in.csv"
    src.write_text(span_csv([("a.txt", 0, 10, 3)]))
    prefix = str(tmp_path / "m")
    assert main(["matrix", str(src), prefix, "--cells"]) == 0
    assert read(matrix.cells_filename(prefix, 6)) == \
        "FILENAME,PHRASE_INDEX,ORIGINAL_SCRIPT_WORD_INDEX,PHRASE,COUNT\r\n"
