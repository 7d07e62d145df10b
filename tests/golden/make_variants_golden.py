#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py variants`.  The committed match CSVs have no
script word with two fan spellings, so this generator writes a small one of its own through
csv.writer and has the test oracle (tests/variants_restated.py) say what the command gives:

  variants_mixed.in.csv                 the records (with the header row)
  variants_mixed.<case>.variants.csv    the cells under the options of <case>
  variants_mixed.<case>.words.csv       ... and the script words

CASES lists (case, --top, --min-records, --fold-case); the tests read the same list.  The
input holds script words with 1, 2, 3, 4 and 70 spellings, a tie in RECORDS that WORKS breaks
(word 13), a tie in both that first appearance breaks (word 14), spellings with a comma, a
doubled quote, non-ASCII text and nothing at all (word 15), Luke / luke / LUKE (word 10), and
a work that comes back later in the file (a.txt).

Run from the repo root:  python tests/golden/make_variants_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "variants_mixed.in.csv"
CASES = [("default", 10, 1, False), ("all_fold", 0, 1, True), ("top3_min2", 3, 2, False)]
KINDS = ("variants", "words")
SCRIPT = {10: ("luke", "VADER", "3"), 11: ("i", "VADER", "3"), 12: ("father", "VADER", "3"),
          13: ("feeling", "HAN", "4"), 14: ("bad", "HAN", "4"), 15: ("this", "HAN", "4"),
          20: ("force", "OBI-WAN", "7, later")}


def golden_names(case):
    return tuple("variants_mixed.%s.%s.csv" % (case, kind) for kind in KINDS)


def records():
    """(work file, script word, fan word) in file order."""
    a, b, c, d = "a.txt", "b.txt", "dir/c.txt", "d.txt"
    out = [(a, 10, "Luke"), (a, 11, "i"), (a, 12, "father"), (a, 13, "feelin"), (a, 13, "feelin"),
           (a, 14, "terrible"), (a, 15, "this,"), (a, 10, "luke"), (a, 12, "dad"),
           (b, 10, "Luke"), (b, 11, "i"), (b, 12, "father"), (b, 13, "sense"), (b, 14, "awful"),
           (b, 15, 'say "this"'), (b, 15, ""), (b, 10, "LUKE"), (b, 14, "bad"),
           (c, 10, "Luke"), (c, 11, "i"), (c, 12, "father"), (c, 13, "sense"), (c, 14, "bad"),
           (c, 15, "thïs → 中"), (c, 15, "this"), (c, 12, "dad"), (c, 10, "luke")]
    # 70 spellings of one word, 1 to 5 records each, over three works
    for k in range(70):
        for j in range(k % 5 + 1):
            out.append(((b, c, d)[(k + j) % 3], 20, "force%02d" % (69 - k)))
    # a.txt comes back
    out += [(a, 11, "i"), (a, 12, "father"), (a, 12, "father"), (a, 14, "bad"), (a, 15, ""),
            (a, 20, "force"), (a, 20, "force"), (a, 20, "force"), (a, 20, "Force"),
            (d, 15, "this"), (d, 20, "force"), (d, 12, "father")]
    return out


def input_csv():
    from tests import passages_restated as pr
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, o, fan in records():
        at[name] = at.get(name, -1) + 1 + (o % 3)
        word, char, scene = SCRIPT[o]
        exact = fan == word
        w.writerow([name, at[name], fan, 100 + len(fan), o, word, 200 + o, char, scene,
                    0.0 if exact else 0.0625, 0 if exact else 2, 0.0 if exact else 0.125])
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import variants_restated
    text = input_csv()
    out = {INPUT: text}
    for case, top, min_records, fold in CASES:
        for name, part in zip(golden_names(case),
                              variants_restated.variants_csv(text, top, min_records, fold)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
