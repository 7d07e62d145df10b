#!/usr/bin/env python3
"""Expected `ao3.py groups` outputs, written by the test oracle (tests/groups_restated.py) for
committed match CSVs and the hand-written metadata groups_meta_spans.csv (getmeta's format; one
work of the inputs has no row, one row has no work):

  groups_<case>.m<M>g<G>.<by>.groups.csv   the groups of <input> with --min-words M --max-gap G
  groups_<case>.m<M>g<G>.<by>.scenes.csv   --by <by> --min-works 1, the group x scene cells
  groups_<case>.m<M>g<G>.<by>.words.csv    and the (group, script word) rows

CASES lists (case, input file under tests/golden, M, G, by): the inputs of
make_quotes_golden.py, each by year, tag and tag:Relationship; the tests read the same list.

Run from the repo root:  python tests/golden/make_groups_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_quotes_golden   # noqa: E402

META = "groups_meta_spans.csv"
BYS = ("year", "tag", "tag:Relationship")
CASES = [(case, src, m, g, by)
         for case, src, m, g in dict.fromkeys(c[:4] for c in make_quotes_golden.CASES)
         for by in BYS]
KINDS = ("groups", "scenes", "words")


def golden_names(case, m, g, by):
    return tuple("groups_%s.m%dg%d.%s.%s.csv" % (case, m, g, by.replace(":", "-"), kind)
                 for kind in KINDS)


def main():
    from tests import groups_restated
    with open(os.path.join(HERE, META), newline="", encoding="utf-8") as fh:
        meta = fh.read()
    for case, src, m, g, by in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        outs = groups_restated.groups_csv(text, meta, by, m, g, 1)
        for name, out in zip(golden_names(case, m, g, by), outs):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows", len(out), "bytes")


if __name__ == "__main__":
    main()
