#!/usr/bin/env python3
"""Expected `ao3.py clusters` outputs, written by the test oracle (tests/clusters_restated.py)
for committed match CSVs:

  clusters_<case>.m<M>g<G>s<S>j<J>z<Z>c<P>.clusters.csv   the families of <input> with
  clusters_<case>.m<M>g<G>s<S>j<J>z<Z>c<P>.works.csv      --min-words M --max-gap G --min-shared S
                                                          --min-jaccard J --min-size Z --common P,
                                                          and its works

CASES lists (case, input file under tests/golden, M, G, S, J, Z, P): the inputs of
make_pairs_golden.py's CASES, each under two settings of the link rule; the tests read the same
list.

Run from the repo root:  python tests/golden/make_clusters_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import make_pairs_golden   # noqa: E402

# (S, J, Z, P): every pair `pairs` keeps at S = 1 as a link and a word common when every member
# covers it (synthetic_small: two listed families and two active works outside them); and the
# command's defaults but for single works, which are listed
SETTINGS = [(1, 0, 2, 100), (6, 50, 1, 50)]
CASES = [(case, src, m, g) + st
         for case, src, m, g in dict.fromkeys(c[:4] for c in make_pairs_golden.CASES)
         for st in SETTINGS]
KINDS = ("clusters", "works")


def golden_names(case, m, g, s, j, z, p):
    return tuple("clusters_%s.m%dg%ds%dj%dz%dc%d.%s.csv" % (case, m, g, s, j, z, p, kind)
                 for kind in KINDS)


def main():
    from tests import clusters_restated
    for case, src, m, g, s, j, z, p in CASES:
        with open(os.path.join(HERE, src), newline="", encoding="utf-8") as fh:
            text = fh.read()
        outs = clusters_restated.clusters_csv(text, m, g, s, j, z, p)
        for name, out in zip(golden_names(case, m, g, s, j, z, p), outs):
            with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
                fh.write(out)
            print(name, out.count("\r\n") - 1, "rows", len(out), "bytes")


if __name__ == "__main__":
    main()
