"""tests/matrix_restated.py (the rules fs_matrix is written from) against
fandom_search_amd.matrix.StrictNgramDedupe: the counter and the kept (work, start) list are
equal on every committed matrix input and on files of the shapes the span rule turns on."""

import glob
import os

import pytest

from fandom_search_amd import matrix
from tests import matrix_cases, matrix_restated as mr, util

INPUTS = sorted(glob.glob(os.path.join(util.GOLDEN, "matrix_*.in.csv")) +
                glob.glob(os.path.join(util.GOLDEN, "matrix_engine", "*.in.csv")))


def check(path, n):
    dd = matrix.StrictNgramDedupe(path, n)
    raw = mr.read_records(path)
    names = list(dict.fromkeys(w for w, _, _ in raw))
    spans, starts, kept = mr.matrix(mr.sort_records(raw), n)
    assert {s: c for s, c in enumerate(starts) if c} == dict(dd.starts_counter)
    assert [(names[w], s) for w, s in kept] == \
        [(m[0]['FAN_WORK_FILENAME'], int(m[0]['ORIGINAL_SCRIPT_WORD_INDEX']))
         for m in dd.filtered_matches]
    assert len(spans) == sum(len(dd.segment_full(rows)) for rows in dd.work_matches.values())
    return len(kept)


def test_inputs_exist():
    assert len(INPUTS) >= 7


@pytest.mark.parametrize("path", INPUTS, ids=[os.path.basename(p) for p in INPUTS])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6])
def test_committed_inputs(path, n):
    check(path, n)


@pytest.mark.parametrize("name", sorted(matrix_cases.shaped()))
def test_shaped_files(name, tmp_path):
    path = str(tmp_path / "in.csv")
    mr.write_csv(path, matrix_cases.shaped()[name])
    kept = sum(check(path, n) for n in (1, 2, 3, 4))
    assert kept


def test_random_files(tmp_path):
    path = str(tmp_path / "in.csv")
    kept = 0
    for seed in range(300):
        mr.write_csv(path, matrix_cases.random_records(seed))
        kept += check(path, 1 + seed % 4)
    assert kept > 300


def test_span_rule_by_hand():
    run = [(0, k, o) for k, o in enumerate([4, 5, 5, 6, 8, 8, 8])]
    assert mr.run_spans(run) == [(4, 5), (5, 6), (8, 8), (8, 8), (8, 8)]
    assert mr.run_spans([(0, 0, 10), (0, 1, 12), (0, 2, 11)]) == [(10, 12)]
