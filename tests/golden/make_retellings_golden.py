#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py retellings`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/retellings_restated.py)
say what the command gives:

  retellings_works.in.csv                  the records (with the header row)
  retellings_works.<case>.retellings.csv   the listed works under the options of <case>
  retellings_works.<case>.passages.csv     ... and their passages

CASES lists (case, --min-words, --max-gap, --min-passages, --min-share); the tests read the
same list.  The input holds a dozen works: a clean retelling (a.txt), the same lines scrambled
(b.txt), a work that repeats a line (c.txt), one without a passage (d.txt), one with a single
passage, one that runs backwards, one whose quotations bridge a word (kept under --max-gap 1),
two interleaved sequences of equal weight, a retelling with one line out of place, a work that
comes back later in the file (j.txt), fan words with a comma, a doubled quote and non-ASCII
text, and a scene whose name holds a comma.

Run from the repo root:  python tests/golden/make_retellings_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "retellings_works.in.csv"
CASES = [("default", 6, 0, 2, 0), ("gap1_min1", 6, 1, 1, 0), ("share80", 6, 0, 2, 80)]
KINDS = ("retellings", "passages")
LINES = {100: ("i have a very bad feeling about this", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "9"),
         160: ("do or do not there is no try", "YODA", "12"),
         180: ("i am altogether ready to go now", "LEIA", "12"),
         200: ("it is a trap get out now", "ACKBAR", "15")}


def golden_names(case):
    return tuple("retellings_works.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def line(at, **changed):
    """The fan words of the line at script word `at`; changed: w<k>=word (None: no record)."""
    words = LINES[at][0].split()
    for key, word in changed.items():
        words[int(key[1:])] = word
    return (at, words)


def quotations():
    """(work file, (first script word, fan words; None: no record for that script word)) in
    file order."""
    a, b, c, d, e, f = "a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt"
    g, h, i, j, k, m = "g.txt", "h.txt", "i.txt", "j.txt", "k.txt", "l.txt"
    return (
        [(a, line(at)) for at in (100, 120, 140, 160, 180, 200)]
        + [(j, line(100)), (j, line(140, w0="Never"))]
        + [(b, line(at)) for at in (200, 160, 100, 180, 120, 140)]
        + [(c, line(100)), (c, line(120)), (c, line(100, w0="I")), (c, line(140))]
        + [(d, (100, "i have a".split())), (d, (160, "do or do not".split()))]
        + [(e, line(160))]
        + [(f, line(at)) for at in (200, 180, 160)]
        + [(g, line(100, w2=None)), (g, line(160)), (g, line(200, w3=None))]
        + [(h, line(at)) for at in (160, 100, 180, 120)]
        + [(i, line(at)) for at in (100, 120, 200, 140, 160)]
        + [(k, line(120, w4="with,", w5='y"ou')), (k, line(200, w6="nöw → 中"))]
        + [(m, (100, "i have a very bad feeling".split())), (m, line(140)), (m, line(120))]
        + [(j, line(120)), (j, line(180)), (j, line(200))])


def input_csv():
    from tests import retellings_restated as rt
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(rt.MATCH_FIELDS)
    at = {}
    for name, (first, fans) in quotations():
        at[name] = at.get(name, 0) + 3                   # words without a record in between
        for k, fan in enumerate(fans):
            at[name] += 1
            if fan is None:
                continue
            word, char, scene = words[first + k]
            exact = fan == word
            w.writerow([name, at[name], fan, 100 + len(fan), first + k, word, 200 + first + k,
                        char, scene, 0.0 if exact else 0.0625, 0 if exact else 2,
                        0.0 if exact else 0.125])
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import retellings_restated as rt
    text = input_csv()
    out = {INPUT: text}
    for case, min_words, max_gap, min_passages, min_share in CASES:
        for name, part in zip(golden_names(case),
                              rt.retellings_csv(text, min_words, max_gap, min_passages,
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
