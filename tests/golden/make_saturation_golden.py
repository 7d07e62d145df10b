#!/usr/bin/env python3
"""The expected outputs of `ao3.py saturation` over the match CSV of the `intervals` goldens,
intervals_lines.in.csv (tests/golden/make_intervals_golden.py describes it; it is read here and
never written).  The test oracle (tests/saturation_restated.py) says what the command gives:

  saturation_lines.<case>.saturation.csv     every point of the curve under the options of <case>
  saturation_lines.<case>.permutations.csv   ... every order
  saturation_lines.<case>.summary.csv        ... and the summary row

CASES lists (case, --by, --min-words, --max-gap, --min-works, --permutations, --points, --seed,
--level); the tests read the same list.  `default` is the command without options; the other two
keep their orders and points few so that the files stay small.

Run from the repo root:  python tests/golden/make_saturation_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "intervals_lines.in.csv"
CASES = [("default", "word", 6, 0, 1, 1000, 100, 0, 95),
         ("scene", "scene", 6, 0, 1, 64, 10, 7, 90),
         ("region_gap1", "region", 6, 1, 1, 40, 7, 3, 99)]
KINDS = ("saturation", "permutations", "summary")


def golden_names(case):
    return tuple("saturation_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def build():
    """{file name: text} of everything this generator writes."""
    from tests import saturation_restated as sr
    with open(os.path.join(HERE, INPUT), newline="", encoding="utf-8") as fh:
        text = fh.read()
    out = {}
    for case, by, min_words, max_gap, min_works, permutations, points, seed, level in CASES:
        for name, part in zip(golden_names(case),
                              sr.saturation_csv(text, by, min_words, max_gap, min_works,
                                                permutations, points, seed, level)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
