#!/usr/bin/env python3
"""Expected `ao3.py works` outputs, written by the test oracle (tests/works_restated.py) for
committed match CSVs:

  works_<case>.m<M>g<G>.works.csv        the per-work summary of <input> with --min-words M
  works_<case>.m<M>g<G>.scenes.csv       --max-gap G, its work x scene cells
  works_<case>.m<M>g<G>.characters.csv   and its work x character cells

CASES lists (case, input file under tests/golden, M, G): the list of make_passages_golden.py;
the tests read the same list.

Run from the repo root:  python tests/golden/make_works_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden.make_passages_golden import CASES   # noqa: E402,F401

KINDS = ("works", "scenes", "characters")


def golden_names(case, m, g):
    return tuple("works_%s.m%dg%d.%s.csv" % (case, m, g, kind) for kind in KINDS)


def main():
    from tests import works_restated
    for case, src, m, g in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        for name, out in zip(golden_names(case, m, g), works_restated.works_csv(text, m, g)):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows")


if __name__ == "__main__":
    main()
