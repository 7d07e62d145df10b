#!/usr/bin/env python3
"""The expected outputs of `ao3.py bundles`.  The inputs are match CSVs other generators of
this directory wrote (contrast_lines.in.csv, retellings_works.in.csv), read and not modified;
the test oracle (tests/bundles_restated.py) says what the command gives:

  bundles_<input>.<case>.bundles.csv   the printed sets under the options of <case>
  bundles_<input>.<case>.units.csv     ... every unit
  bundles_<input>.<case>.levels.csv    ... and every size 2 .. --max-size + 1

CASES lists (input, case, --by, --min-words, --max-gap, --min-works, --min-all, --max-size,
--all); the tests read the same list.  `deep` reaches the lone set of six units of the
retellings fixture, with levels 7 to 9 empty; in `gap1_size3` the unprinted level 4 does the
marking of level 3.

Run from the repo root:  python tests/golden/make_bundles_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

CONTRAST, RETELLINGS = "contrast_lines.in.csv", "retellings_works.in.csv"
CASES = [(CONTRAST, "default", "region", 6, 0, 1, 5, 4, False),
         (CONTRAST, "all2", "region", 6, 0, 1, 2, 4, True),
         (RETELLINGS, "deep", "region", 6, 0, 1, 2, 8, False),
         (RETELLINGS, "gap1_size3", "region", 6, 1, 1, 2, 3, True),
         (CONTRAST, "scene", "scene", 6, 0, 1, 5, 4, False)]
KINDS = ("bundles", "units", "levels")


def golden_names(source, case):
    stem = source[:-len(".in.csv")]
    return tuple("bundles_%s.%s.%s.csv" % (stem, case, kind) for kind in KINDS)


def build():
    """{file name: text} of everything this generator writes."""
    from tests import bundles_restated as br
    out = {}
    for source, case, by, min_words, max_gap, min_works, min_all, max_size, every in CASES:
        with open(os.path.join(HERE, source), newline="", encoding="utf-8") as fh:
            text = fh.read()
        for name, part in zip(golden_names(source, case),
                              br.bundles_csv(text, by, min_words, max_gap, min_works, min_all,
                                             max_size, every)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
