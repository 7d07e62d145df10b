#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py intervals`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/intervals_restated.py)
say what the command gives:

  intervals_lines.in.csv                  the records (with the header row)
  intervals_lines.<case>.intervals.csv    every unit under the options of <case>
  intervals_lines.<case>.replicates.csv   ... and every replicate

CASES lists (case, --by, --min-words, --max-gap, --min-works, --replicates, --seed, --level); the
tests read the same list.  The script has five lines; scene 4 holds the first and the third.
Thirty-two works: two in three quote the first line; every fourth quotes the second and the
third line, the same works both, units that tie in every replicate; two in five the fourth;
every sixth the fifth with a word left out, a passage only under --max-gap 1, where that word,
which no record names, is a unit of --by word with the text [?].  A work that quotes none of
them has three stray words: it is in the file, so it is resampled, and it is not active.
w00.txt comes back at the end of the file; a scene name holds a comma.

Run from the repo root:  python tests/golden/make_intervals_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "intervals_lines.in.csv"
CASES = [("default", "region", 6, 0, 1, 1000, 0, 95),
         ("scene", "scene", 6, 0, 1, 64, 7, 90),
         ("word_gap1", "word", 6, 1, 1, 40, 0, 95)]
KINDS = ("intervals", "replicates")
N_WORKS = 32
LINES = {100: ("i have a bad feeling about", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "4"),
         160: ("do or do not there is", "YODA", "12"),
         180: ("it is a trap get out now", "ACKBAR", "15")}


def golden_names(case):
    return tuple("intervals_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


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
    out = []
    for i in range(N_WORKS):
        name = "w%02d.txt" % i
        mine = []
        if i % 3 != 2 and i % 10 != 9:
            mine.append(line(100))
        if i % 4 == 0:
            mine += [line(120), line(140)]
        if i % 5 in (1, 2):
            mine.append(line(160))
        if i % 6 == 1:
            mine.append(line(180, skip=2))
        if not mine:
            mine.append(line(100, words=3))
        out += [(name, q) for q in mine]
    return out + [("w00.txt", line(160))]


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
    from tests import intervals_restated as ir
    text = input_csv()
    out = {INPUT: text}
    for case, by, min_words, max_gap, min_works, replicates, seed, level in CASES:
        for name, part in zip(golden_names(case),
                              ir.intervals_csv(text, by, min_words, max_gap, min_works,
                                               replicates, seed, level)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
