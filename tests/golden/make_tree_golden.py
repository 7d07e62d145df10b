#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py tree`.  This generator writes a small match CSV
of its own, built by hand below, through csv.writer and has the test oracle
(tests/tree_restated.py), not the library, say what the command gives:

  tree_lines.in.csv             the records (with the header row)
  tree_lines.<case>.tree.csv    the merges under the options of <case>
  tree_lines.<case>.works.csv   ... the active works
  tree_lines.<case>.levels.csv  ... and the levels

CASES lists (case, command-line options, the oracle's keywords); the tests read the same list.
Twelve works over seven lines of the script.  The input holds:
  a.txt and b.txt with identical coverage (lines 0 and 10): the first merge, at 1000000; under
      the defaults g.txt and l.txt are identical too, g.txt's five words of line 50 being no
      passage;
  dir/c.txt (lines 0 and 20) and d.txt (lines 10 and 20): d.txt shares seven words with each of
      a.txt, b.txt and dir/c.txt, 7 of 22 each time, a tie between three edges of different
      pairs; the one with the earliest work A, a.txt, is the merge;
  a second tree of five works, e.txt to h.txt and l.txt, larger than the first and so ranked
      before it although it appears later; under --measure shared the edges a.txt -- dir/c.txt,
      e.txt -- g.txt and e.txt -- l.txt all merge at eight shared words, ties across the trees;
  i.txt, which quotes a line nobody else does and joins nothing;
  j.txt with a run of five words, a passage only from --min-words 5 down, which then shares
      five words with g.txt and h.txt, fewer than --min-shared 6: a second tree of one work;
  k.txt stepping over "bad" of line 0: a passage under --max-gap 1, 8 of 15 with each of a.txt,
      b.txt and dir/c.txt; a.txt -- k.txt merges, b.txt -- k.txt finds one family, dir/c.txt --
      k.txt merges next at the same level;
  e.txt -- h.txt, 6 of 22 under --min-words 4, which --min-level 300000 drops while f.txt --
      h.txt, 6 of 14, stays;
  a.txt coming back later in the file.

Run from the repo root:  python tests/golden/make_tree_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "tree_lines.in.csv"
CASES = [("defaults", [], {}),
         ("shared_s2", ["--measure", "shared", "--min-shared", "2"],
          dict(measure="shared", min_shared=2)),
         ("gap1_words4_level300000",
          ["--max-gap", "1", "--min-words", "4", "--min-level", "300000"],
          dict(max_gap=1, min_words=4, min_level=300000))]
KINDS = ("tree", "works", "levels")
LINES = {0: ("i have a very bad feeling about this", "HAN", "4"),
         10: ("may the force be with you always", "OBI-WAN", "7, later"),
         20: ("i find your lack of faith disturbing", "VADER", "9"),
         30: ("these are not the droids you are looking for", "OBI-WAN", "12"),
         40: ("do or do not there is no try", "YODA", "21"),
         50: ("never tell me the odds", "HAN", "23"),
         60: ("help me obi-wan kenobi you are my only hope", "LEIA", "2")}


def golden_names(case):
    return tuple("tree_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def quotations():
    """(work file, first script word, words, offsets without a record) in file order."""
    a, b, c, d, e, f, g, h, i, j, k, l = (
        "a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt", "g.txt", "h.txt", "i.txt",
        "j.txt", "k.txt", "l.txt")
    return [
        (a, 0, 8, ()), (b, 0, 8, ()), (b, 10, 7, ()),
        (c, 0, 8, ()), (c, 20, 7, ()),
        (d, 10, 7, ()), (d, 20, 7, ()),
        (e, 30, 9, ()), (e, 40, 8, ()),
        (f, 30, 9, ()),
        (g, 40, 8, ()), (g, 50, 5, ()),
        (h, 50, 5, ()), (h, 30, 6, ()),
        (i, 60, 9, ()),
        (j, 50, 5, ()),
        (k, 0, 8, (4,)),
        (l, 40, 8, ()),
        (a, 10, 7, ()),
    ]


def input_csv():
    from tests import passages_restated as pr
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, first, n, skipped in quotations():
        at[name] = at.get(name, 0) + 3                   # words without a record in between
        for k in range(n):
            at[name] += 1
            if k in skipped:
                continue
            word, char, scene = words[first + k]
            w.writerow([name, at[name], word, 100 + len(word), first + k, word, 200 + first + k,
                        char, scene, 0.0, 0, 0.0])
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import tree_restated
    text = input_csv()
    out = {INPUT: text}
    for case, _, kw in CASES:
        for name, part in zip(golden_names(case), tree_restated.tree_csv(text, **kw)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
