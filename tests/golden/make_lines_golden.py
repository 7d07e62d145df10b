#!/usr/bin/env python3
"""The inputs and the expected outputs of `ao3.py lines`.  This generator writes a small script
markup and a match CSV of its own through csv.writer and has the test oracle
(tests/lines_restated.py) say what the command gives:

  lines_speeches.markup.txt           the script: twelve lines, three characters, three scenes
  lines_speeches.in.csv               the records (with the header row)
  lines_speeches.<case>.lines.csv     the lines under the options of <case>
  lines_speeches.<case>.works.csv     ... the works
  lines_speeches.<case>.cells.csv     ... and the cells

CASES lists (case, --min-words, --max-gap, --min-works, --most); the tests read the same list.
The first line stands before any character or scene tag; a `LINE<<>>` without a token is no
line; the third scene tag has no digit, so the scene is the count of scene tags from there.
Eight works: a and g quote "i have a bad feeling about this" whole, b its first six words, c its
last six; c quotes the last line twice (once counted); d runs from the second word of "you are
who" through "i am luke skywalker" to the third word of the next line; e quotes the long line in
two pieces; f leaves a word out of "what an incredible smell ...", a passage only under
--max-gap 1, which completes the line; h has a stray three words; a.txt comes back at the end of
the file with two whole lines in one passage.

Run from the repo root:  python tests/golden/make_lines_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

MARKUP = "lines_speeches.markup.txt"
INPUT = "lines_speeches.in.csv"
CASES = [("default", 6, 0, 1, 50), ("gap1_most80", 6, 1, 1, 80), ("minworks2", 6, 0, 2, 50)]
KINDS = ("lines", "works", "cells")
SCRIPT = """LINE<<a long time ago>>
SCENE_NUMBER<<4>>
CHARACTER_NAME<<HAN>>
LINE<<i have a bad feeling about this>>
LINE<<>>
CHARACTER_NAME<<LEIA>>
LINE<<would somebody get this big walking carpet out of my way before i shoot>>
CHARACTER_NAME<<HAN>>
LINE<<no reward is worth this>>
SCENE_NUMBER<<7>>
CHARACTER_NAME<<LUKE>>
LINE<<i am here to rescue you>>
CHARACTER_NAME<<LEIA>>
LINE<<you are who>>
DIRECTION<<He takes off the helmet>>
CHARACTER_NAME<<LUKE>>
LINE<<i am luke skywalker>>
LINE<<i have got your droids>>
SCENE_NUMBER<<INT. TRASH COMPACTOR>>
CHARACTER_NAME<<HAN>>
LINE<<what an incredible smell you have discovered>>
CHARACTER_NAME<<LEIA>>
LINE<<it could be worse>>
CHARACTER_NAME<<HAN>>
LINE<<it is worse>>
CHARACTER_NAME<<LUKE>>
LINE<<may the force be with you>>
"""
# the 1-based lines the quotations name
BAD_FEELING, CARPET, WHO, DROIDS, SMELL, COULD, IS_WORSE, FORCE = 2, 3, 6, 8, 9, 10, 11, 12


def golden_names(case):
    return tuple("lines_speeches.%s.%s.csv" % (case, kind) for kind in KINDS)


def quotations(line_first):
    """(work file, script words with a record) in file order."""
    def words(line, a=0, b=None, skip=None):
        """Words a .. b - 1 of the 1-based line (b None: to its end), without word `skip`."""
        at, end = line_first[line - 1], line_first[line]
        b = end - at if b is None else b
        return [at + k for k in range(a, b) if k != skip]
    a, b, c, d, e, f, g, h = ("a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt", "g.txt",
                              "h.txt")
    through = list(range(line_first[WHO - 1] + 1, line_first[DROIDS - 1] + 3))
    return ([(a, words(BAD_FEELING)), (a, words(FORCE))]
            + [(b, words(BAD_FEELING, 0, 6)), (b, words(FORCE))]
            + [(c, words(FORCE)), (c, words(BAD_FEELING, 1)), (c, words(FORCE))]
            + [(d, through)]
            + [(e, words(CARPET, 0, 6)), (e, words(CARPET, 8))]
            + [(f, words(SMELL, skip=3))]
            + [(g, words(FORCE)), (g, words(BAD_FEELING))]
            + [(h, words(CARPET, 2, 5))]
            + [(a, words(COULD) + words(IS_WORSE))])


def input_csv():
    from tests import lines_restated as lr
    from tests import passages_restated as pr
    script, line_first = lr.markup_lines(SCRIPT)
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, ws in quotations(line_first):
        base = at.get(name, 0) + 3                       # words without a record in between
        for o in ws:
            word, char, scene = script[o]
            fan = word.upper() if (o - ws[0]) == 1 else word
            exact = fan == word
            w.writerow([name, base + o - ws[0], fan, 100 + len(fan), o, word, 200 + o, char, scene,
                        0.0 if exact else 0.0625, 0 if exact else 2, 0.0 if exact else 0.125])
        at[name] = base + ws[-1] - ws[0]
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import lines_restated as lr
    text = input_csv()
    out = {MARKUP: SCRIPT, INPUT: text}
    for case, min_words, max_gap, min_works, most in CASES:
        for name, part in zip(golden_names(case),
                              lr.lines_csv(text, SCRIPT, min_words, max_gap, min_works, most)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
