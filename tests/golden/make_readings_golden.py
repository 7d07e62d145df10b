#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py readings`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/readings_restated.py)
say what the command gives:

  readings_lines.in.csv                 the records (with the header row)
  readings_lines.<case>.readings.csv    the readings under the options of <case>
  readings_lines.<case>.spans.csv       ... and the spans

CASES lists (case, --min-words, --max-gap, --top, --min-works, --fold-case); the tests read the
same list.  The input holds a line that several works quote verbatim, with its last word, its
first word or only its case changed, one work repeating it, a quotation that is a prefix of
it, the same fan words at two places of the script, quotations that bridge different words of
one span (kept under --max-gap 1), fan words with a comma, a doubled quote and non-ASCII
text, and a work that comes back later in the file (a.txt).

Run from the repo root:  python tests/golden/make_readings_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "readings_lines.in.csv"
CASES = [("default", 6, 0, 10, 1, False), ("all_fold", 6, 0, 0, 1, True),
         ("gap1_top2_min2", 4, 1, 2, 2, False)]
KINDS = ("readings", "spans")
LINES = {100: ("i have a very bad feeling about this", "HAN", "4"),
         110: ("may the force be with you always", "OBI-WAN", "7, later"),
         120: ("never tell me the odds", "HAN", "9"),
         130: ("may the force be with you", "LEIA", "12")}


def golden_names(case):
    return tuple("readings_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def quotations():
    """(work file, first script word, fan words; None: no record for that script word) in
    file order."""
    a, b, c, d, e, f = "a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt"
    bad = "i have a very bad feeling about this".split()
    may = "may the force be with you".split()
    return [
        (a, 100, ["I"] + bad[1:]), (a, 110, may), (a, 130, may),
        (b, 100, bad), (b, 110, may[:2] + ["Force", "be", "with", "ya"]),
        (c, 100, bad[:7] + ["that"]), (c, 110, may[:5] + ["us"]),
        (d, 100, bad), (d, 100, bad), (d, 110, ["May"] + may[1:]), (d, 100, bad[:6]),
        (e, 100, ["we"] + bad[1:]), (e, 110, may), (e, 110, may + ["always"]),
        (e, 120, ["never", "tell", None, "the", "odds"]),
        (f, 120, ["never", None, "me", "the", "odds"]),
        (f, 120, "never tell me the odds".split()),
        (f, 110, may[:4] + ["with,", 'y"ou']), (f, 130, may[:5] + ["yoü → 中"]),
        (b, 120, ["Never", "tell", None, "the", "odds"]), (c, 130, may),
        (a, 100, bad), (a, 120, ["never", "tell", None, "the", "odds"]),
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
    from tests import readings_restated
    text = input_csv()
    out = {INPUT: text}
    for case, min_words, max_gap, top, min_works, fold in CASES:
        for name, part in zip(golden_names(case),
                              readings_restated.readings_csv(text, min_words, max_gap, top,
                                                             min_works, fold)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
