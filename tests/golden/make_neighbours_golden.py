#!/usr/bin/env python3
"""Expected `ao3.py neighbours` outputs, written by the test oracle (tests/neighbours_restated.py)
for a committed match CSV:

  neighbours_<case>.neighbours.csv   each work's closest works
  neighbours_<case>.works.csv        the works
  neighbours_<case>.words.csv        depth and weight of the covered script words

INPUT is companions_lines.in.csv (make_companions_golden.py writes it): eight works over a few
lines, which under the defaults gives the weights 1, 2 and 3 and works whose candidates tie on
SIMILARITY_PPM; contrast_lines.in.csv gives the same three weights and ten times the rows.
CASES lists (case, the command's options, the oracle's keywords); the tests read the same list.

Run from the repo root:  python tests/golden/make_neighbours_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "companions_lines.in.csv"
CASES = [("defaults", [], {}),
         ("flat_top3", ["--weight", "flat", "--top", "3"], dict(weight="flat", top=3)),
         ("gap1_sim50_top1", ["--max-gap", "1", "--min-similarity", "50", "--top", "1"],
          dict(max_gap=1, min_similarity=50, top=1))]
KINDS = ("neighbours", "works", "words")


def golden_names(case):
    return tuple("neighbours_%s.%s.csv" % (case, kind) for kind in KINDS)


def main():
    from tests import neighbours_restated
    with open(os.path.join(HERE, INPUT), newline="", encoding="utf-8") as fh:
        text = fh.read()
    for case, _, kw in CASES:
        outs = neighbours_restated.neighbours_csv(text, **kw)
        for name, out in zip(golden_names(case), outs):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows", len(out), "bytes")


if __name__ == "__main__":
    main()
