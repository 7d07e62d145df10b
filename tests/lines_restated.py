"""The `lines` contract restated in plain Python on tests/companions_restated.py's coverage: a
set of script words per work, a loop over the lines, a loop over the works.  The oracle of
tests/test_lines_host.py and tests/test_gpu_lines.py and of the committed
tests/golden/lines_*.csv.  The product never imports it."""

import csv
import io
import re

from fandom_search_amd import vocab
from tests import companions_restated as cr
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
LINE_FIELDS = ['LINE', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'WORDS', 'CHARACTER', 'SCENE',
               'WORKS', 'WHOLE_WORKS', 'MOST_WORKS', 'HEAD_WORKS', 'TAIL_WORKS',
               'MEAN_SHARE_PERCENT', 'WHOLE_PERCENT', 'FIRST_FAN_WORK_FILENAME', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'LINES', 'WHOLE_LINES', 'COVERED_WORDS', 'LINE_WORDS',
               'SHARE_PERCENT', 'TOP_LINE', 'TOP_LINE_COVERED', 'TOP_LINE_WORDS', 'TOP_LINE_TEXT']
CELL_FIELDS = ['LINE', 'FAN_WORK_FILENAME', 'COVERED_WORDS', 'LINE_WORDS', 'SHARE_PERCENT',
               'FIRST_COVERED_WORD_INDEX', 'LAST_COVERED_WORD_INDEX', 'RUNS', 'WHOLE',
               'SPAN_TEXT']
LINE_KEYS = ['works', 'whole_works', 'most_works', 'head_works', 'tail_works', 'first_work',
             'covered_sum']
WORK_KEYS = ['work', 'lines', 'whole_lines', 'covered', 'line_words', 'top_line', 'top_covered']
CELL_KEYS = ['line', 'work', 'covered', 'first', 'last', 'runs']


def markup_lines(text):
    """(words, line_first) of a markup's text: per script word (lower-case word, character,
    scene), and the word each line starts at with the number of words behind them.  A text line
    is a scene tag, else a character tag, else a LINE tag; a LINE without a token is no line; a
    scene label keeps its digits, and from the first label without any the scene is the number
    of scene tags so far."""
    words, line_first = [], []
    scene = character = None
    tags, counting = 0, False
    for t in text.splitlines():
        m = re.search('SCENE_NUMBER<<([^>]*)>>', t)
        if m:
            tags += 1
            digits = ''.join(ch for ch in m.group(1) if ch.isdigit())
            try:
                scene = int(digits)
            except ValueError:                       # none, or digits int() does not read
                counting = True
            if counting:
                scene = tags
            continue
        m = re.search('CHARACTER_NAME<<([^>]*)>>', t)
        if m:
            character = m.group(1)
            continue
        m = re.search('LINE<<([^>]*)>>', t)
        if m:
            toks = [tok.lower() for tok in vocab.tokenize(m.group(1))]
            if toks:
                line_first.append(len(words))
                words += [(w, character, scene) for w in toks]
    return words, line_first + [len(words)]


def lines(records, n_works, n_script, line_first, min_words=6, max_gap=0, most=50):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).  Returns (one
    dict of LINE_KEYS per line, one of WORK_KEYS per active work in work order, one of CELL_KEYS
    per cell in (line, work) order)."""
    if min_words < 1 or not 1 <= most <= 100:
        raise ValueError("min_words must be at least 1, most 1 to 100")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    n_lines = len(line_first) - 1
    if n_lines and records:
        if line_first[0] != 0 or line_first[-1] != n_script or \
                any(line_first[l] >= line_first[l + 1] for l in range(n_lines)):
            raise ValueError("lines that do not tile the script")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = cr.coverage(records, n_works, min_words, max_gap) if n_lines else []
    active = [w for w in range(n_works) if n_lines and cov[w]]
    out_lines, out_cells = [], []
    per_work = {w: dict(work=w, lines=0, whole_lines=0, covered=0, line_words=0, top_line=NONE,
                        top_covered=0) for w in active}
    for l in range(n_lines):
        a, b = line_first[l], line_first[l + 1] - 1
        size = b - a + 1
        row = dict(works=0, whole_works=0, most_works=0, head_works=0, tail_works=0,
                   first_work=NONE, covered_sum=0)
        for w in active:
            inside = [o for o in range(a, b + 1) if o in cov[w]]
            if not inside:
                continue
            n = len(inside)
            runs = sum(1 for k, o in enumerate(inside) if k == 0 or inside[k - 1] != o - 1)
            out_cells.append(dict(line=l, work=w, covered=n, first=inside[0], last=inside[-1],
                                  runs=runs))
            row['works'] += 1
            row['whole_works'] += n == size
            row['most_works'] += n * 100 >= most * size
            row['head_works'] += inside[0] == a
            row['tail_works'] += inside[-1] == b
            row['covered_sum'] += n
            if row['first_work'] == NONE:
                row['first_work'] = w
            v = per_work[w]
            v['lines'] += 1
            v['whole_lines'] += n == size
            v['covered'] += n
            v['line_words'] += size
            if n > v['top_covered']:                 # the earlier line on a tie
                v['top_line'], v['top_covered'] = l, n
        out_lines.append(row)
    return out_lines, [per_work[w] for w in active], out_cells


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def lines_csv(text, markup_text, min_words=6, max_gap=0, min_works=1, most=50):
    """The bytes `ao3.py lines` writes for a match CSV's text and a markup's text: (lines,
    lines-works, lines-cells)."""
    if not 1 <= most <= 100:
        raise ValueError("--most %d: a whole percentage from 1 to 100" % most)
    words, line_first = markup_lines(markup_text)
    n_script = len(words)
    rows = pr.read_rows(text)
    work_of, keyed = {}, []
    for k, r in enumerate(rows):
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    names = list(work_of)
    far = max([int(r[4]) for r in rows], default=-1)
    if far >= n_script:
        raise ValueError("ORIGINAL_SCRIPT_WORD_INDEX %d in a script markup of %d words (the "
                         "records need at least %d): was the file searched against another "
                         "script?" % (far, n_script, far + 1))
    wrong = sorted((int(r[4]), k) for k, r in enumerate(rows) if r[5] != words[int(r[4])][0])
    if wrong:
        o, k = wrong[0]
        raise ValueError("script word %d is %r in the records and %r in the script markup: "
                         "was the file searched against another script?"
                         % (o, rows[k][5], words[o][0]))
    found, per_work, cells = lines(recs, len(names), n_script, line_first, min_words, max_gap,
                                   most)

    def text_of(a, b):
        return ' '.join(words[o][0] for o in range(a, b + 1))

    def size(l):
        return line_first[l + 1] - line_first[l]
    ltab = [LINE_FIELDS]
    kept = [l for l in range(len(found)) if found[l]['works'] >= min_works]
    for l in sorted(kept, key=lambda l: (-found[l]['works'], -found[l]['whole_works'], l)):
        v, a, b = found[l], line_first[l], line_first[l + 1] - 1
        n = v['works']
        ltab.append([l + 1, a, b, size(l), words[a][1], words[a][2], n, v['whole_works'],
                     v['most_works'], v['head_works'], v['tail_works'],
                     v['covered_sum'] * 100 // (n * size(l)) if n else 0,
                     v['whole_works'] * 100 // n if n else 0,
                     '' if v['first_work'] == NONE else names[v['first_work']], text_of(a, b)])
    wtab = [WORK_FIELDS]
    for v in per_work:
        top = v['top_line']
        wtab.append([names[v['work']], v['lines'], v['whole_lines'], v['covered'],
                     v['line_words'], v['covered'] * 100 // v['line_words'], top + 1,
                     v['top_covered'], size(top),
                     text_of(line_first[top], line_first[top + 1] - 1)])
    ctab = [CELL_FIELDS]
    for v in cells:
        n, k = v['covered'], size(v['line'])
        ctab.append([v['line'] + 1, names[v['work']], n, k, n * 100 // k, v['first'], v['last'],
                     v['runs'], 1 if n == k else 0, text_of(v['first'], v['last'])])
    return _csv(ltab), _csv(wtab), _csv(ctab)
