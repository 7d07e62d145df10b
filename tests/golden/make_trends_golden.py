#!/usr/bin/env python3
"""The expected outputs of `ao3.py trends`.  The inputs are those of `contrast`
(contrast_lines.in.csv and contrast_lines.meta.csv, tests/golden/make_contrast_golden.py: eight
script lines, forty-eight works dated 2014 to 2017, w46.txt without a date, w47.txt without a
metadata row, works that quote no line in the file and in the pool and not active); the test
oracle (tests/trends_restated.py) says what the command gives:

  trends_lines.<case>.trends.csv          the family's units under the options of <case>
  trends_lines.<case>.periods.csv         ... the works of every period
  trends_lines.<case>.permutations.csv    ... and every re-dating

CASES lists (case, --by, --unit, --min-words, --max-gap, --min-works, --min-quoting,
--permutations, --seed); the tests read the same list, and the README's three example commands
are these.

Run from the repo root:  python tests/golden/make_trends_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "contrast_lines.in.csv"
META = "contrast_lines.meta.csv"
CASES = [("year", "year", "region", 6, 0, 1, 5, 1000, 0),
         ("month_scene", "month", "scene", 6, 0, 1, 5, 64, 7),
         ("word_gap1", "year", "word", 6, 1, 1, 3, 40, 0)]
KINDS = ("trends", "periods", "permutations")


def golden_names(case):
    return tuple("trends_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def build():
    """{file name: text} of everything this generator writes."""
    from tests import trends_restated as tr
    with open(os.path.join(HERE, INPUT), newline="", encoding="utf-8") as fh:
        text = fh.read()
    with open(os.path.join(HERE, META), newline="", encoding="utf-8") as fh:
        meta = fh.read()
    out = {}
    for case, by, unit, m, g, k, q, P, seed in CASES:
        for name, part in zip(golden_names(case),
                              tr.trends_csv(text, meta, by, unit, m, g, k, q, P, seed)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
