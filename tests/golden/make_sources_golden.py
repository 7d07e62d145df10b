#!/usr/bin/env python3
"""The inputs and the expected outputs of `ao3.py sources`.  This generator writes three small
match CSVs of its own through csv.writer, one corpus searched against the three scripts of a
trilogy, and has the test oracle (tests/sources_restated.py) say what the command gives:

  sources_trilogy.<a|b|c>.in.csv           the records of script a, b, c (with the header row)
  sources_trilogy.<case>.sources.csv       the passages under the options of <case>
  sources_trilogy.<case>.works.csv         ... the (work, script) rows
  sources_trilogy.<case>.scripts.csv       ... the scripts
  sources_trilogy.<case>.pairs.csv         ... and the pairs of scripts

CASES lists (case, --min-words, --max-gap); the tests read the same list.  The scripts are
named hope, empire and jedi (--names).  All three hold "may the force be with you always";
hope and empire share "i have a bad feeling about this".  Thirteen works:
  a.txt      quotes the line all three share, every word exact: the earlier script wins
  b.txt      the line two share, a word misspelt in hope's file: empire wins on exact words
  dir/c.txt  a line of hope alone (a file name with a slash)
  d.txt      the chain: hope's twelve words, empire's eight on the last two of them, jedi's six
             on the last of those; jedi loses to a passage that lost itself
  e.txt      lines of hope and of jedi far apart; the work is missing from empire's file
  f.txt, g.txt  the shared line; empire's file lists g before f, so that its own order of first
             appearance is not the shared numbering
  h.txt      the line all share, a word without a record in jedi's file: a passage of jedi
             only under --max-gap 1
  i.txt      the line all share twice, the second time not in jedi
  j.txt      in jedi's file only, in the middle of it: numbered last
  k.txt      empire's six words nested in hope's twelve
  l.txt      a line of hope and a line of jedi adjacent: no rivals
  m.txt      the same two lines touching in one word: rivals
The scene of hope's shared line holds a comma.

Run from the repo root:  python tests/golden/make_sources_golden.py
"""

import csv
import io
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SCRIPTS = ("a", "b", "c")
NAMES = ["hope", "empire", "jedi"]
CASES = [("default", 6, 0), ("gap1", 6, 1)]
KINDS = ("sources", "works", "scripts", "pairs")
FORCE = "may the force be with you always"
FEELING = "i have a bad feeling about this"
CHAIN = ("you do not know the power of the dark side i must obey my master he will show you "
         "the true nature of").split()
LONG = "the force is strong with this one i can feel it now".split()
# per script {line: (first script word, text, character, scene)}
LINES = {
    "a": {"force": (100, FORCE, "OBI-WAN", "7, later"),
          "feeling": (120, FEELING, "HAN", "4"),
          "odds": (140, "never tell me the odds kid", "HAN", "9"),
          "chain": (160, " ".join(CHAIN[0:12]), "VADER", "12"),
          "long": (200, " ".join(LONG), "VADER", "14")},
    "b": {"force": (50, FORCE, "YODA", "3"),
          "feeling": (70, FEELING, "HAN", "5"),
          "chain": (90, " ".join(CHAIN[10:18]), "VADER", "8"),
          "nest": (130, " ".join(LONG[3:9]), "EMPEROR", "10")},
    "c": {"force": (10, FORCE, "LUKE", "1"),
          "chain": (30, " ".join(CHAIN[17:23]), "EMPEROR", "2"),
          "flown": (50, "kid i have flown from one", "HAN", "6"),
          "own": (70, "it is a trap get out", "ACKBAR", "15")},
}


def q(work, fan, line, skip=None, inexact=()):
    return (work, fan, line, skip, tuple(inexact))


# per script, in file order: (work, first fan word, line, the word without a record, the words
# spelt otherwise in the fan work)
QUOTES = {
    "a": [q("a.txt", 10, "force"), q("b.txt", 5, "feeling", inexact=[2]),
          q("dir/c.txt", 3, "odds"), q("d.txt", 0, "chain"), q("e.txt", 4, "odds"),
          q("f.txt", 2, "feeling"), q("g.txt", 8, "feeling"), q("h.txt", 6, "force"),
          q("i.txt", 1, "force"), q("i.txt", 30, "force"), q("k.txt", 20, "long"),
          q("l.txt", 0, "odds"), q("m.txt", 0, "odds")],
    "b": [q("a.txt", 10, "force"), q("b.txt", 5, "feeling"), q("d.txt", 10, "chain"),
          q("g.txt", 8, "feeling"), q("f.txt", 2, "feeling"), q("h.txt", 6, "force"),
          q("i.txt", 1, "force"), q("i.txt", 30, "force", inexact=[0]), q("k.txt", 23, "nest")],
    "c": [q("a.txt", 10, "force"), q("d.txt", 17, "chain"), q("e.txt", 40, "own"),
          q("h.txt", 6, "force", skip=3), q("i.txt", 1, "force"), q("j.txt", 0, "own"),
          q("j.txt", 20, "flown"), q("l.txt", 6, "flown"), q("m.txt", 5, "flown")],
}


def input_name(script):
    return "sources_trilogy.%s.in.csv" % script


def golden_names(case):
    return tuple("sources_trilogy.%s.%s.csv" % (case, kind) for kind in KINDS)


def input_csv(script):
    from tests import passages_restated as pr
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(pr.MATCH_FIELDS)
    for work, fan, line, skip, inexact in QUOTES[script]:
        first, text, char, scene = LINES[script][line]
        for k, word in enumerate(text.split()):
            if k == skip:
                continue
            exact = k not in inexact
            spelt = word if exact else word.upper()
            w.writerow([work, fan + k, spelt, 100 + len(spelt), first + k, word, 200 + first + k,
                        char, scene, 0.0 if exact else 0.0625, 0 if exact else 2,
                        0.0 if exact else 0.125])
    return buf.getvalue()


def arguments(case):
    """The command line of a CASES entry, behind the inputs and -o."""
    _, min_words, max_gap = case
    return ["--names", ",".join(NAMES), "--min-words", str(min_words), "--max-gap", str(max_gap)]


def build():
    """{file name: text} of everything this generator writes."""
    from tests import sources_restated as sr
    texts = [input_csv(s) for s in SCRIPTS]
    out = {input_name(s): t for s, t in zip(SCRIPTS, texts)}
    for case, min_words, max_gap in CASES:
        for name, part in zip(golden_names(case), sr.sources_csv(texts, NAMES, min_words, max_gap)):
            out[name] = part
    return out


def main():
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
