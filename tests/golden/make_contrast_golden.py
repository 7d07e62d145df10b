#!/usr/bin/env python3
"""The inputs and the expected outputs of `ao3.py contrast`.  This generator writes a small
match CSV and a metadata CSV of its own through csv.writer and has the test oracle
(tests/contrast_restated.py) say what the command gives:

  contrast_lines.in.csv                     the records (with the header row)
  contrast_lines.meta.csv                   a metadata row per work but one
  contrast_lines.<case>.contrast.csv        the family's units under the options of <case>
  contrast_lines.<case>.sides.csv           ... the four sides
  contrast_lines.<case>.permutations.csv    ... and every permutation

CASES lists (case, --by, --a keys, --b keys, --unit, --min-words, --max-gap, --min-works,
--min-quoting, --permutations, --seed); the tests read the same list, and the README's three
example commands are these.  The script has eight lines.  Forty-eight works; every third is
tagged Alternate Universe.  Twelve of those sixteen and three of the other thirty-two quote the
first line: the planted difference, which no relabelling of 1000 reaches (GE = ADJ_GE = 0).
Nine of the sixteen and seven of the others quote the fourth line: alone it passes at 5 %
(P_PPM 32 967), among the lines of the family it does not (ADJ_PPM 119 880).  The other lines are
quoted by works picked without regard to the tag.  w47.txt has
no metadata row; w46.txt has no date; a work that quotes no line has three stray words, so it is
in the file and in the pool and it is not active.  A scene name holds a comma.

Run from the repo root:  python tests/golden/make_contrast_golden.py
"""

import csv
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "contrast_lines.in.csv"
META = "contrast_lines.meta.csv"
AU = "Alternate Universe"
CASES = [("tag", "tag:Additional Tags", (AU,), (), "region", 6, 0, 1, 5, 1000, 0),
         ("years", "year", ("2016", "2017"), ("2014",), "scene", 6, 0, 1, 5, 64, 7),
         ("language", "language", ("English",), (), "word", 6, 1, 1, 3, 40, 0)]
KINDS = ("contrast", "sides", "permutations")
N_WORKS = 48
LINES = {100: ("i have a bad feeling about", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "4"),
         160: ("do or do not there is", "YODA", "12"),
         180: ("it is a trap get out now", "ACKBAR", "15"),
         200: ("these are not the droids you seek", "OBI-WAN", "7, later"),
         220: ("i find your lack of faith disturbing", "VADER", "9"),
         240: ("the garbage will do just fine", "REY", "21")}


def golden_names(case):
    return tuple("contrast_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def is_au(i):
    return i % 3 == 0


def pick(i, at, out_of, below):
    """A choice that does not look at the tag: a fixed scramble of (work, line)."""
    return ((i * 2654435761 + at * 40503 + 12345) >> 7) % out_of < below


def quotes_line(i, at):
    if at == 100:                                        # twelve of sixteen against three
        return i % 12 != 9 if is_au(i) else i % 11 == 5
    if at == 160:                                        # nine of sixteen against seven
        return i % 6 == 0 or i == 3 if is_au(i) else i % 4 == 1 and i < 40
    if at == 180:
        return pick(i, at, 10, 2)
    return pick(i, at, 10, {120: 4, 140: 3, 200: 5, 220: 3, 240: 2}[at])


def quotations():
    """(work file, first script word, the words of the line with a record) in file order."""
    out = []
    for i in range(N_WORKS):
        name = "w%02d.txt" % i
        mine = []
        for at, (text, _, _) in LINES.items():
            if quotes_line(i, at):
                n = len(text.split())
                mine.append((at, [k for k in range(n) if not (at == 180 and k == 2)]))
        if not mine:
            mine.append((100, [0, 1, 2]))
        out += [(name, at, ks) for at, ks in mine]
    return out


def input_csv():
    from tests import passages_restated as pr
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, first, ks in quotations():
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


def meta_csv():
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(["FILENAME", "TITLE", "AUTHOR", "SUMMARY", "NOTES", "PUBLICATION_DATE", "LANGUAGE",
                "TAGS"])
    for i in range(N_WORKS - 1):                         # (w47 has no row)
        extra = [AU] if is_au(i) else []
        extra.append(("Fluff", "Angst", "Hurt/Comfort", "Humor")[i % 4])
        tags = {"Rating": "General Audiences", "Additional Tags": "; ".join(extra)}
        if i % 5 == 0:
            tags["Relationship"] = "Rey/Finn"
        date = "" if i == 46 else "%d-%02d-%02d" % (2014 + (i * 7 // 3) % 4, 1 + i % 12, 1 + i % 28)
        w.writerow(["w%02d.html" % i, "Story %d" % i, "author%d" % (i % 9), "A summary, with a comma",
                    "", date, ("English", "English", "Deutsch", "English", "Français")[i % 5],
                    json.dumps(tags, ensure_ascii=False)])
    return buf.getvalue()


def build():
    """{file name: text} of everything this generator writes."""
    from tests import contrast_restated as cn
    text, meta = input_csv(), meta_csv()
    out = {INPUT: text, META: meta}
    for case, by, a_keys, b_keys, unit, m, g, k, q, P, seed in CASES:
        for name, part in zip(golden_names(case),
                              cn.contrast_csv(text, meta, by, a_keys, b_keys, unit, m, g, k, q, P,
                                              seed)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
