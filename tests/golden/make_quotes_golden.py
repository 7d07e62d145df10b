#!/usr/bin/env python3
"""Expected `ao3.py quotes` outputs, written by the test oracle (tests/quotes_restated.py) for
committed match CSVs:

  quotes_<case>.m<M>g<G>k<K>.quotes.csv   the regions of <input> with --min-words M --max-gap G
  quotes_<case>.m<M>g<G>k<K>.words.csv    --min-works K, and its script words

CASES lists (case, input file under tests/golden, M, G, K): the matrix_spans_a/b/c,
synthetic_small and synthetic_n4 cases of make_works_golden.py, each at K = 1 and K = 2; the
tests read the same list.

Run from the repo root:  python tests/golden/make_quotes_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_works_golden   # noqa: E402

NAMES = ("matrix_spans_a", "matrix_spans_b", "matrix_spans_c", "synthetic_small", "synthetic_n4")
CASES = [(case, src, m, g, k) for case, src, m, g in make_works_golden.CASES if case in NAMES
         for k in (1, 2)]
KINDS = ("quotes", "words")


def golden_names(case, m, g, k):
    return tuple("quotes_%s.m%dg%dk%d.%s.csv" % (case, m, g, k, kind) for kind in KINDS)


def main():
    from tests import quotes_restated
    for case, src, m, g, k in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        outs = quotes_restated.quotes_csv(text, m, g, k)
        for name, out in zip(golden_names(case, m, g, k), outs):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows", len(out), "bytes")


if __name__ == "__main__":
    main()
