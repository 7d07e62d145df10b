#!/usr/bin/env python3
"""The input and the expected outputs of `ao3.py transitions`.  This generator writes a small
match CSV of its own through csv.writer and has the test oracle (tests/transitions_restated.py)
say what the command gives:

  transitions_lines.in.csv                   the records (with the header row)
  transitions_lines.<case>.transitions.csv   the kept cells under the options of <case>
  transitions_lines.<case>.units.csv         ... and every unit

CASES lists (case, --by, --min-words, --max-gap, --min-works, --within, --min-steps,
--min-step-works, --min-share), None for a --within left out; the tests read the same list.  The
script has six lines; scene 4 holds the first and the third (a label that comes back: one scene
unit).  Twelve works: a walks forward through five lines and b through three (b.txt comes back
at the end of the file with a fourth); c jumps back from the fourth line to the first; d repeats
the first line before going on (a loop); e has a single passage; f opens on a line nobody else
quotes, which is no region under --min-works 2, so its sequence starts one passage later there;
g leaves nine fan words between its two passages, more than --within 5; h and i quote the fifth
line with a word left out, a passage only under --max-gap 1; j walks the last three lines; k has
three stray words in front; l goes from the first line to the third, a loop under --by scene.  A
scene name holds a comma, a file name a slash.

Run from the repo root:  python tests/golden/make_transitions_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

INPUT = "transitions_lines.in.csv"
CASES = [("default", "region", 6, 0, 1, None, 1, 2, 0),
         ("scene", "scene", 6, 0, 1, None, 1, 2, 0),
         ("gap1_within5_share50", "region", 6, 1, 2, 5, 1, 2, 50)]
KINDS = ("transitions", "units")
LINES = {100: ("i have a bad feeling about", "HAN", "4"),
         120: ("may the force be with you always", "OBI-WAN", "7, later"),
         140: ("never tell me the odds kid", "HAN", "4"),
         160: ("do or do not there is", "YODA", "12"),
         180: ("it is a trap get out now", "ACKBAR", "15"),
         200: ("these are not the droids you want", "OBI-WAN", "20")}
GAP = 3                     # fan words without a record between two quotations of a work


def golden_names(case):
    return tuple("transitions_lines.%s.%s.csv" % (case, kind) for kind in KINDS)


def script():
    """{script word index: (word, character, scene)}."""
    return {at + k: (w, char, scene) for at, (text, char, scene) in LINES.items()
            for k, w in enumerate(text.split())}


def line(at, skip=None, words=None, gap=GAP):
    """The script words a work quotes of the line at `at` (all, all but word `skip`, or the
    first `words`) and the fan words without a record in front."""
    n = len(LINES[at][0].split())
    return (at, [k for k in range(n if words is None else words) if k != skip], gap)


def quotations():
    """(work file, (first script word, the words of the line with a record, the fan words in
    front)) in file order."""
    a, b, c, d, e, f = "a.txt", "b.txt", "dir/c.txt", "d.txt", "e.txt", "f.txt"
    g, h, i, j, k, m = "g.txt", "h.txt", "i.txt", "j.txt", "k.txt", "l.txt"
    return ([(a, line(at)) for at in (100, 120, 140, 160, 180)]
            + [(b, line(100)), (b, line(120)), (b, line(140))]
            + [(c, line(160)), (c, line(100)), (c, line(120))]
            + [(d, line(100)), (d, line(100)), (d, line(120))]
            + [(e, line(120))]
            + [(f, line(200)), (f, line(100)), (f, line(120))]
            + [(g, line(100)), (g, line(140, gap=9))]
            + [(h, line(160)), (h, line(180, skip=2))]
            + [(i, line(180, skip=2)), (i, line(160))]
            + [(j, line(140)), (j, line(160, gap=5)), (j, line(180, gap=6))]
            + [(k, line(100, words=3)), (k, line(120)), (k, line(140))]
            + [(m, line(100)), (m, line(140))]
            + [(b, line(160))])


def input_csv():
    from tests import passages_restated as pr
    words = script()
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    at = {}
    for name, (first, ks, gap) in quotations():
        base = at.get(name, 0) + gap
        for k in ks:
            word, char, scene = words[first + k]
            fan = word.upper() if k == 1 else word
            exact = fan == word
            w.writerow([name, base + 1 + k, fan, 100 + len(fan), first + k, word, 200 + first + k,
                        char, scene, 0.0 if exact else 0.0625, 0 if exact else 2,
                        0.0 if exact else 0.125])
        at[name] = base + 1 + max(ks)
    return buf.getvalue()


def options(case):
    """The restatement's keyword arguments of a CASES entry."""
    _, by, min_words, max_gap, min_works, within, min_steps, min_step_works, min_share = case
    return dict(by=by, min_words=min_words, max_gap=max_gap, min_works=min_works,
                within=0xFFFFFFFF if within is None else within, min_steps=min_steps,
                min_step_works=min_step_works, min_share=min_share)


def arguments(case):
    """The command line of a CASES entry, behind the input and -o."""
    _, by, min_words, max_gap, min_works, within, min_steps, min_step_works, min_share = case
    argv = ["--by", by, "--min-words", str(min_words), "--max-gap", str(max_gap),
            "--min-works", str(min_works), "--min-steps", str(min_steps),
            "--min-step-works", str(min_step_works), "--min-share", str(min_share)]
    return argv if within is None else argv + ["--within", str(within)]


def build():
    """{file name: text} of everything this generator writes."""
    from tests import transitions_restated as tr
    text = input_csv()
    out = {INPUT: text}
    for case in CASES:
        for name, part in zip(golden_names(case[0]), tr.transitions_csv(text, **options(case))):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
