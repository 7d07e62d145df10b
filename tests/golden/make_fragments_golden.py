#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py fragments`.  This generator writes a match CSV
of its own through csv.writer over the script of make_lines_golden.py and has the test oracle
(tests/fragments_restated.py) say what the command gives:

  fragments_speeches.in.csv                 the records (with the header row)
  fragments_speeches.<case>.fragments.csv   the fragments under the options of <case>
  fragments_speeches.<case>.works.csv       ... and the works

CASES lists (case, --min-words, --max-gap, --min-works, --min-length, --max-words, --top); the
tests read the same list.  Ten works:
  a, g  "i have a bad feeling about this" whole; b its first six words, c its last six: the five
        words in the middle are a fragment of four works inside fragments of three and of two
  a, b  begin at the script's word 0 ("a long time ago i have ...")
  a, b, c, g  "may the force be with you", the script's last words; c quotes it twice
  e     the long line in two passages that abut: one run; i quotes it in one passage, and only
        the run makes the whole line a fragment of two works
  f, j  "what an incredible smell ..." without its fourth word: passages only under --max-gap 1,
        and then a fragment with a word no record names
  h     a stray three words

Run from the repo root:  python tests/golden/make_fragments_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "fragments_speeches.in.csv"
CASES = [("default", 6, 0, 2, 3, 128, 0), ("gap1_min1", 6, 1, 1, 1, 128, 0),
         ("top3", 6, 0, 2, 3, 128, 3)]
KINDS = ("fragments", "works")


def golden_names(case):
    return tuple("fragments_speeches.%s.%s.csv" % (case, kind) for kind in KINDS)


def quotations(line_first):
    """(work file, script words with a record) in file order."""
    from tests.golden.make_lines_golden import BAD_FEELING, CARPET, FORCE, SMELL

    def words(line, a=0, b=None, skip=None):
        at, end = line_first[line - 1], line_first[line]
        b = end - at if b is None else b
        return [at + k for k in range(a, b) if k != skip]
    a, b, c, e, f, g, h, i, j = ("a.txt", "b.txt", "dir/c.txt", "e.txt", "f.txt", "g.txt",
                                 "h.txt", "i.txt", "j.txt")
    opening = list(range(0, line_first[BAD_FEELING - 1]))
    return ([(a, opening + words(BAD_FEELING)), (a, words(FORCE))]
            + [(b, opening + words(BAD_FEELING, 0, 6)), (b, words(FORCE))]
            + [(c, words(FORCE)), (c, words(BAD_FEELING, 1)), (c, words(FORCE))]
            + [(e, words(CARPET, 0, 6)), (e, words(CARPET, 6))]
            + [(f, words(SMELL, skip=3))]
            + [(g, words(FORCE)), (g, words(BAD_FEELING))]
            + [(h, words(CARPET, 2, 5))]
            + [(i, words(CARPET))]
            + [(j, words(SMELL, skip=3))])


def input_csv():
    from tests import lines_restated as lr
    from tests import passages_restated as pr
    from tests.golden.make_lines_golden import SCRIPT
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
    from tests import fragments_restated as fr
    text = input_csv()
    out = {INPUT: text}
    for case, min_words, max_gap, min_works, min_length, max_words, top in CASES:
        for name, part in zip(golden_names(case),
                              fr.fragments_csv(text, min_words, max_gap, min_works, min_length,
                                               max_words, top)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
