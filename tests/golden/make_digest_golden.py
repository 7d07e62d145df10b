#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py digest`.  This generator writes a small match
CSV of its own, by hand, through csv.writer, and has the test oracle (tests/digest_restated.py)
say what the command gives:

  digest_speeches.in.csv               the records (with the header row)
  digest_speeches.<case>.digest.csv    the picks under the options of <case>
  digest_speeches.<case>.works.csv     ... and the works

CASES lists (case, --min-words, --max-gap, --picks, --cover, --min-gain); the tests read the
same list.  Three speeches of 19, 14 and 15 words and twelve works:
  a, b  the first sixteen words of the first speech: two identical works, and only the first
        is ever picked
  c     its first ten words: contained in a
  d     the second speech without its eighth word, in two passages: a pick with two new runs
  e     the end of the first speech and the start of the second, in two passages with another
        work's records between them in the file: it overlaps a and d and adds three words to
        them, as many as k, which comes later in the file
  f, h  the third speech without its fifth word, which no record names: f words 1..4 and 6..11,
        h all the others.  Under --max-gap 0 the first four words are no passage; under
        --max-gap 1 the fifth word is bridged, and h's new run holds a word without a text
  g     the last nine words of the third speech
  i     a stray three words: no passage
  j     the first six words of the second speech: contained in d and in e
  k     the last seven words of the first speech and seven of the third
  l     the last seven words of the second speech, in a file under a directory: the one word
        d leaves out makes it the last pick

Run from the repo root:  python tests/golden/make_digest_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "digest_speeches.in.csv"
CASES = [("default", 6, 0, 0, 100, 1), ("gap1_cover80", 6, 1, 0, 80, 1),
         ("picks2", 6, 0, 2, 100, 1)]
KINDS = ("digest", "works")
SPEECHES = [("HAMLET", "1", "to be or not to be that is the question whether tis nobler in the "
                            "mind to suffer the"),
            ("MACBETH", "2", "tomorrow and tomorrow and tomorrow creeps in this petty pace from "
                             "day to day"),
            ("PORTIA", "3", "the quality of mercy is not strained it droppeth as the gentle rain "
                            "from heaven")]
FIRST = (0, 19, 33, 48)             # the first script word of each speech, and the script's length
BRIDGED = 37                        # "is" of the third speech: no record names it


def golden_names(case):
    return tuple("digest_speeches.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """(word, character, scene) per script word."""
    out = [(w, char, scene) for char, scene, text in SPEECHES for w in text.split()]
    assert len(out) == FIRST[3]
    return out


def quotations():
    """(work file, script words with a record) in file order."""
    def words(a, b):
        return [o for o in range(a, b + 1) if o != BRIDGED]
    return [("a.txt", words(0, 15)), ("e.txt", words(11, 18)), ("b.txt", words(0, 15)),
            ("c.txt", words(0, 9)), ("d.txt", words(19, 25)), ("d.txt", words(27, 32)),
            ("e.txt", words(19, 25)), ("f.txt", words(33, 43)), ("g.txt", words(39, 47)),
            ("h.txt", words(33, 47)), ("i.txt", words(26, 28)), ("j.txt", words(19, 24)),
            ("k.txt", words(12, 18)), ("k.txt", words(40, 46)), ("dir/l.txt", words(26, 32))]


def input_csv():
    from tests import passages_restated as pr
    text = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, ws in quotations():
        base = at.get(name, 0) + 3                       # words without a record in between
        for o in ws:
            word, char, scene = text[o]
            fan = word.upper() if (o - ws[0]) == 1 else word
            exact = fan == word
            w.writerow([name, base + o - ws[0], fan, 100 + len(fan), o, word, 200 + o, char, scene,
                        0.0 if exact else 0.0625, 0 if exact else 2, 0.0 if exact else 0.125])
        at[name] = base + ws[-1] - ws[0]
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import digest_restated as dr
    text = input_csv()
    out = {INPUT: text}
    for case, min_words, max_gap, picks, cover, min_gain in CASES:
        for name, part in zip(golden_names(case),
                              dr.digest_csv(text, min_words, max_gap, picks, cover, min_gain)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
