#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py companions`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/companions_restated.py)
say what the command gives:

  companions_lines.in.csv                  the records (with the header row)
  companions_lines.<case>.companions.csv   the kept pairs under the options of <case>
  companions_lines.<case>.units.csv        ... and every unit

CASES lists (case, --by, --min-words, --max-gap, --min-works, --min-both, --min-share); the tests
read the same list.  The script has five lines; scene 4 holds the first and the third (a label
that comes back: one scene unit).  Nine works: a, b and c quote the first line with the second or
the third (c the first line twice: once counted); d and i quote the fifth line with a word left
out, a passage only under --max-gap 1, where that word, which no record names, is in the region
and in no scene; e has a stray three words; g and a quote the first and the fourth line, two of
the five works of each, a pair --min-share 50 drops; a.txt comes back at the end of the file; a
scene name holds a comma, a file name a slash.

Run from the repo root:  python tests/golden/make_companions_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "companions_lines.in.csv"
CASES = [("default", "region", 6, 0, 1, 2, 0), ("scene", "scene", 6, 0, 1, 2, 0),
         ("gap1_share50", "region", 6, 1, 1, 2, 50)]
KINDS = ("companions", "units")
LINES = {100: ("i have a bad feeling about", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "4"),
         160: ("do or do not there is", "YODA", "12"),
         180: ("it is a trap get out now", "ACKBAR", "15")}


def golden_names(case):
    return tuple("companions_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def line(at, skip=None, words=None):
    """The script words a work quotes of the line at `at`: all, all but word `skip`, or the
    first `words`."""
    n = len(LINES[at][0].split())
    return (at, [k for k in range(n if words is None else words) if k != skip])


def quotations():
    """(work file, (first script word, the words of the line with a record)) in file order."""
    a, b, c, d, e = "a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt"
    f, g, h, i = "f.txt", "g.txt", "h.txt", "i.txt"
    return ([(a, line(100)), (a, line(120))]
            + [(b, line(100)), (b, line(120)), (b, line(140))]
            + [(c, line(100)), (c, line(140)), (c, line(100))]
            + [(d, line(160)), (d, line(180, skip=2))]
            + [(e, line(100, words=3))]
            + [(f, line(140)), (f, line(160))]
            + [(g, line(160)), (g, line(100))]
            + [(h, line(100))]
            + [(i, line(180, skip=2)), (i, line(160))]
            + [(a, line(160))])


def input_csv():
    from tests import passages_restated as pr
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, (first, ks) in quotations():
        at[name] = at.get(name, 0) + 3                   # words without a record in between
        base = at[name]
        for k in ks:
            word, char, scene = words[first + k]
            fan = word.upper() if k == 1 else word
            exact = fan == word
            w.writerow([name, base + 1 + k, fan, 100 + len(fan), first + k, word, 200 + first + k,
                        char, scene, 0.0 if exact else 0.0625, 0 if exact else 2,
                        0.0 if exact else 0.125])
        at[name] = base + 1 + max(ks)
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import companions_restated as cr
    text = input_csv()
    out = {INPUT: text}
    for case, by, min_words, max_gap, min_works, min_both, min_share in CASES:
        for name, part in zip(golden_names(case),
                              cr.companions_csv(text, by, min_words, max_gap, min_works, min_both,
                                                min_share)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
