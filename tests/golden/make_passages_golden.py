#!/usr/bin/env python3
"""Expected `ao3.py passages` outputs, written by the test oracle (tests/passages_restated.py)
for committed match CSVs:

  passages_<case>.m<M>g<G>.csv   the passage CSV of <input> with --min-words M --max-gap G

CASES lists (case, input file under tests/golden, M, G); the tests read the same list.

Run from the repo root:  python tests/golden/make_passages_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CASES = [
    ("synthetic_small", "synthetic_small.literal.csv", 6, 0),      # batch file: no header
    ("synthetic_small", "synthetic_small.literal.csv", 6, 1),
    ("synthetic_n4", "synthetic_n4.literal.csv", 4, 0),
    ("matrix_synthetic_small", "matrix_synthetic_small.in.csv", 6, 0),   # dated file: header
    ("matrix_spans_a", "matrix_spans_a.in.csv", 6, 0),
    ("matrix_spans_b", "matrix_spans_b.in.csv", 4, 0),
    ("matrix_spans_b", "matrix_spans_b.in.csv", 4, 2),
    ("matrix_spans_c", "matrix_spans_c.in.csv", 3, 0),
]


def golden_name(case, m, g):
    return "passages_%s.m%dg%d.csv" % (case, m, g)


def main():
    sys.path.insert(0, ROOT)
    from tests import passages_restated
    for case, src, m, g in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        out = passages_restated.passages_csv(text, m, g)
        with open(os.path.join(HERE, golden_name(case, m, g)), "w", newline="",
                  encoding="utf-8") as fh:
            fh.write(out)
        print(golden_name(case, m, g), out.count("\r\n") - 1, "passages")


if __name__ == "__main__":
    main()
