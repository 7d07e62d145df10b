#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py misquotes`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/misquotes_restated.py)
say what the command gives:

  misquotes_lines.in.csv                 the records (with the header row)
  misquotes_lines.<case>.misquotes.csv   the listed misquotes under the options of <case>
  misquotes_lines.<case>.pairs.csv       ... the kept pairs
  misquotes_lines.<case>.works.csv       ... and the active works

CASES lists (case, command-line options, the oracle's keywords); the tests read the same list.
The input holds:
  "that" for "this" in a.txt and b.txt, which also share "thé → 中" for "the" with h.txt: two
      shared misquotes of one weight, the tie of the strongest;
  "disturbin," (a comma) for "disturbing" in a.txt and dir/c.txt, two of the four works that
      quote the word: telling exactly at --max-share 50;
  "forse" for "force" in five of the seven works that quote it: not telling at 50;
  "ya" for "you" in d.txt and e.txt, two of eight: a heavier weight than the others;
  "May" and "I", departures only under --keep-case;
  "that" again in g.txt inside a run of five words, kept from --min-words 5 down;
  f.txt stepping over "bad" (kept under --max-gap 1), where three works write "baad": f.txt is
      no reader of that word;
  a one-off "four" in e.txt, and a.txt coming back later in the file.

Run from the repo root:  python tests/golden/make_misquotes_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "misquotes_lines.in.csv"
CASES = [("defaults", [], {}),
         ("keepcase_flat_share100", ["--keep-case", "--weight", "flat", "--max-share", "100"],
          dict(keep_case=True, weight="flat", max_share=100)),
         ("gap1_words4_works3_shared2",
          ["--max-gap", "1", "--min-words", "4", "--min-works", "3", "--min-shared", "2"],
          dict(max_gap=1, min_words=4, min_works=3, min_shared=2))]
KINDS = ("misquotes", "pairs", "works")
LINES = {100: ("i have a very bad feeling about this", "HAN", "4"),
         110: ("may the force be with you always", "OBI-WAN", "7, later"),
         120: ("i find your lack of faith disturbing", "VADER", "9"),
         130: ("these are not the droids you are looking for", "OBI-WAN", "12")}


def golden_names(case):
    return tuple("misquotes_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def line(at, **changed):
    """The words of the line at `at`, those at the offsets `changed` names (w0, w1, ...)
    replaced; None: no record for that script word."""
    words = LINES[at][0].split()
    for k, fan in changed.items():
        words[int(k[1:])] = fan
    return words


def quotations():
    """(work file, first script word, fan words) in file order."""
    a, b, c, d, e, f, g, h = ("a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt", "g.txt",
                              "h.txt")
    the = "thé → 中"
    return [
        (a, 100, line(100, w7="that")), (a, 110, line(110, w2="forse")),
        (b, 100, line(100, w0="I", w7="that")), (b, 110, line(110, w2="forse")),
        (c, 100, line(100, w4="baad")), (c, 110, line(110, w2="forse")),
        (c, 120, line(120, w6="disturbin,")), (c, 130, line(130)),
        (d, 100, line(100, w4="baad")), (d, 110, line(110, w0="May", w2="forse")),
        (d, 120, line(120)), (d, 130, line(130, w5="ya")),
        (b, 120, line(120)), (b, 130, line(130, w3=the)),
        (e, 100, line(100, w4="baad")), (e, 110, line(110, w0="May", w2="forse")),
        (e, 130, line(130, w5="ya", w8="four")),
        (f, 100, line(100, w4=None)), (f, 110, line(110)), (f, 130, line(130)),
        (g, 103, line(100, w7="that")[3:]), (g, 130, line(130)),
        (h, 130, line(130, w3=the)), (h, 110, line(110)),
        (a, 120, line(120, w6="disturbin,")), (a, 130, line(130, w3=the)),
    ]


def input_csv():
    from tests import passages_restated as pr
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, first, fans in quotations():
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
    from tests import misquotes_restated
    text = input_csv()
    out = {INPUT: text}
    for case, _, kw in CASES:
        for name, part in zip(golden_names(case), misquotes_restated.misquotes_csv(text, **kw)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
