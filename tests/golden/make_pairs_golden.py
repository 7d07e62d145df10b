#!/usr/bin/env python3
"""Expected `ao3.py pairs` outputs, written by the test oracle (tests/pairs_restated.py) for
committed match CSVs:

  pairs_<case>.m<M>g<G>s<S>.pairs.csv   the pairs of <input> with --min-words M --max-gap G
  pairs_<case>.m<M>g<G>s<S>.works.csv   --min-shared S, and its works

CASES lists (case, input file under tests/golden, M, G, S): the inputs of
make_quotes_golden.py, each at S = 1 and S = 6; the tests read the same list.

Run from the repo root:  python tests/golden/make_pairs_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_quotes_golden   # noqa: E402

CASES = [(case, src, m, g, s)
         for case, src, m, g in dict.fromkeys(c[:4] for c in make_quotes_golden.CASES)
         for s in (1, 6)]
KINDS = ("pairs", "works")


def golden_names(case, m, g, s):
    return tuple("pairs_%s.m%dg%ds%d.%s.csv" % (case, m, g, s, kind) for kind in KINDS)


def main():
    from tests import pairs_restated
    for case, src, m, g, s in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        outs = pairs_restated.pairs_csv(text, m, g, s)
        for name, out in zip(golden_names(case, m, g, s), outs):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows", len(out), "bytes")


if __name__ == "__main__":
    main()
