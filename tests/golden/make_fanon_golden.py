#!/usr/bin/env python3
"""The expected outputs of `ao3.py fanon` over tests/golden/fanon_works, nine short fan works
written for this purpose, and the script markup tests/golden/fanon_script.txt.  The test oracle
(tests/fanon_restated.py) says what the command gives:

  fanon.<case>.phrases.csv    PREFIX-fanon.csv under the options of <case>
  fanon.<case>.passages.csv   PREFIX-fanon-passages.csv
  fanon.<case>.grams.csv      PREFIX-fanon-grams.csv
  fanon.<case>.works.csv      PREFIX-fanon-works.csv

CASES lists (case, command-line options, whether the script is given); the tests read the same
list.  The works:
  ashes, binary, dune, gone, hollow
                             open with the same disclaimer (binary in lower case: one phrase
                             unless --keep-case): five works of nine, common under --max-share 50
  ashes, echo                the same story, echo without the disclaimer: a repost
  ashes, binary, comet, echo "hope is a debt the galaxy never repays"; far quotes it broken
  comet, hollow              "may the force be with you, always and forever", which the script
                             holds: canon when the script is given, else shared; far has its
                             first six tokens only
  gone                       a word nine times over: grams that overlap themselves
  empty                      no position
The file names in the CSVs are the paths as the command lists them: run it, and this generator,
from the repo root:  python tests/golden/make_fanon_golden.py
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

WORKS = os.path.join("tests", "golden", "fanon_works")
SCRIPT = os.path.join("tests", "golden", "fanon_script.txt")
CASES = [("default", [], False),
         ("k4_w3_case", ["--length", "4", "--min-works", "3", "--keep-case"], False),
         ("share50_script", ["--max-share", "50"], True)]
KINDS = ("phrases", "passages", "grams", "works")


def golden_names(case):
    return tuple("fanon.%s.%s.csv" % (case, kind) for kind in KINDS)


def restated_options(options):
    """The keyword arguments of fanon_restated.tables for command-line options."""
    args = {}
    for flag, key in (("--length", "length"), ("--min-works", "min_works"),
                      ("--max-share", "max_share"), ("--top", "top")):
        if flag in options:
            args[key] = int(options[options.index(flag) + 1])
    args["keep_case"] = "--keep-case" in options
    return args


def build():
    """{file name: text} of everything this generator writes."""
    from tests import fanon_restated as fr
    out = {}
    for case, options, with_script in CASES:
        parts = fr.tables(WORKS, [SCRIPT] if with_script else [], **restated_options(options))
        for name, head, rows in zip(golden_names(case), fr.HEADS, parts):
            out[name] = fr.csv_text(head, rows)
    return out


def main():
    os.chdir(ROOT)
    for name, text in build().items():
        with open(os.path.join(HERE, name), "w", newline="", encoding="utf-8") as fh:
            fh.write(text)
        print(name, text.count("\r\n") - 1, "rows", len(text.encode("utf-8")), "bytes")


if __name__ == "__main__":
    main()
