#!/usr/bin/env python3
"""The expected outputs of `ao3.py routes`.  The inputs are match CSVs other generators of this
directory wrote (transitions_lines.in.csv, retellings_works.in.csv), read and not modified; the
test oracle (tests/routes_restated.py) says what the command gives:

  routes_<input>.<case>.routes.csv   the printed routes under the options of <case>
  routes_<input>.<case>.units.csv    ... every unit
  routes_<input>.<case>.levels.csv   ... and every length 2 .. --max-length + 1

CASES lists (input, case, --by, --min-words, --max-gap, --min-works, --min-all, --max-length,
--max-skip, --all); the tests read the same list.  `deep` mines to length 9; in `run_all`
--max-skip 0 keeps the contiguous runs only and --all prints the routes that are not closed.

Run from the repo root:  python tests/golden/make_routes_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TRANSITIONS, RETELLINGS = "transitions_lines.in.csv", "retellings_works.in.csv"
CASES = [(TRANSITIONS, "default", "region", 6, 0, 1, 5, 4, None, False),
         (TRANSITIONS, "scene", "scene", 6, 0, 1, 2, 4, None, False),
         (TRANSITIONS, "run_all", "region", 6, 0, 1, 2, 4, 0, True),
         (RETELLINGS, "deep", "region", 6, 0, 1, 2, 8, None, False),
         (RETELLINGS, "run_all", "region", 6, 0, 1, 2, 4, 0, True)]
KINDS = ("routes", "units", "levels")


def golden_names(source, case):
    stem = source[:-len(".in.csv")]
    return tuple("routes_%s.%s.%s.csv" % (stem, case, kind) for kind in KINDS)


def build():
    """{file name: text} of everything this generator writes."""
    from tests import routes_restated as rr
    out = {}
    for source, case, by, min_words, max_gap, min_works, min_all, max_length, skip, every in CASES:
        with open(os.path.join(HERE, source), newline="", encoding="utf-8") as fh:
            text = fh.read()
        parts = rr.routes_csv(text, by, min_words, max_gap, min_works, min_all, max_length,
                              rr.NONE if skip is None else skip, every)
        for name, part in zip(golden_names(source, case), parts):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
