#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py alignments`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/alignments_restated.py)
say what the command gives:

  alignments_lines.in.csv                  the records (with the header row)
  alignments_lines.<case>.alignments.csv   the kept alignments under the options of <case>
  alignments_lines.<case>.works.csv        ... and the works that have one
  alignments_cli.json                      the command's arguments as the command line has them
                                           (the form of cli_surface.json, which pins the
                                           commands of cli.build_parser(); this one is added
                                           behind them by cli.full_parser())

CASES lists (case, --min-words, --reach, --match, --gap); the tests read the same list.  The
input holds a dozen short works: verbatim lines (a.txt), the line with one inserted word that
found a stray match and one dropped word (b.txt), a substituted word with a record and one
without (c.txt), a line whose halves are swapped (d.txt: the script side must advance, so two
alignments), two records at one fan index (e.txt, and a tree with a side record), nothing but
strays (f.txt), fan words with a comma, a doubled quote and non-ASCII text beside a scene whose
name holds a comma (g.txt), a work that comes back later in the file (h.txt), two dropped
script words (i.txt: joined by the default reach, not by --reach 1), three inserted fan words
(j.txt), a quote too short to keep (k.txt) and a last link that costs more than a word scores
(m.txt: the path stops short of it).

Run from the repo root:  python tests/golden/make_alignments_golden.py
"""

import csv
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "alignments_lines.in.csv"
CLI = "alignments_cli.json"
CASES = [("default", 6, 4, 2, 1), ("reach0", 6, 0, 2, 1), ("reach1_gap2", 6, 1, 2, 2)]
KINDS = ("alignments", "works")
LINES = {100: ("i have a very bad feeling about all this", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "9"),
         160: ("do or do not there is no try", "YODA", "12"),
         200: ("it is a trap get out now", "ACKBAR", "15"),
         220: ("help me obi wan kenobi you are my only hope left in the galaxy", "LEIA", "2")}


def golden_names(case):
    return tuple("alignments_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def run(fan, orig, count, **changed):
    """`count` records stepping together from (fan, orig); changed: w<k>=the fan word of the
    k-th of them."""
    recs = [[fan + k, orig + k, None] for k in range(count)]
    for key, word in changed.items():
        recs[int(key[1:])][2] = word
    return [tuple(r) for r in recs]


def records():
    """(work file, [(fan index, script index, fan word; None: the script's word)]) in file
    order."""
    return [
        ("a.txt", run(1, 100, 9) + run(20, 120, 7)),
        ("h.txt", run(5, 140, 6)),
        ("b.txt", run(10, 100, 3) + [(13, 203, "always")] + run(14, 103, 3) + run(17, 107, 2)),
        ("dir/c.txt", run(1, 140, 6, w2="you") + run(21, 160, 3) + run(25, 164, 4)),
        ("d.txt", run(1, 227, 7) + run(8, 220, 7)),
        ("e.txt", run(1, 120, 3) + [(4, 204, "be"), (4, 123, None)] + run(5, 124, 3)
         + run(20, 200, 5) + [(25, 205, None), (25, 206, "now"), (26, 206, None)]),
        ("f.txt", [(1, 200, "it"), (2, 140, "never"), (3, 105, "feeling"), (5, 161, "or"),
                   (8, 122, "force")]),
        ("g.txt", run(3, 120, 7, w4="with,", w5='y"ou') + [(10, 165, "is")]
         + run(11, 200, 7, w6="nöw → 中")),
        ("i.txt", run(1, 220, 5) + run(6, 227, 5)),
        ("j.txt", run(1, 160, 4) + run(8, 164, 4)),
        ("k.txt", run(1, 200, 5)),
        ("m.txt", run(1, 100, 6) + [(10, 108, None)]),
        ("h.txt", run(40, 100, 4) + run(45, 104, 5)),
    ]


def input_csv():
    from tests import alignments_restated as ar
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(ar.MATCH_FIELDS)
    for name, recs in records():
        for fan_ix, orig_ix, fan in recs:
            word, char, scene = words[orig_ix]
            fan = word if fan is None else fan
            exact = fan == word
            w.writerow([name, fan_ix, fan, 100 + len(fan), orig_ix, word, 200 + orig_ix, char,
                        scene, 0.0 if exact else 0.0625, 0 if exact else 2,
                        0.0 if exact else 0.125])
    return buf.getvalue()


def cli_surface():
    """The entry of `alignments` in the surface of cli.full_parser(), which stands last."""
    from fandom_search_amd import cli
    from tests.golden.make_cli_surface import surface
    return json.loads(json.dumps(surface(cli.full_parser())[-1]))


def build():
    """{file name: text} of everything this generator writes."""
    from tests import alignments_restated as ar
    text = input_csv()
    out = {INPUT: text, CLI: json.dumps(cli_surface(), indent=1) + "\n"}
    for case, min_words, reach, match, gap in CASES:
        for name, part in zip(golden_names(case),
                              ar.alignments_csv(text, min_words, reach, match, gap)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
