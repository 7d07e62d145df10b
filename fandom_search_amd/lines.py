"""`ao3.py lines`: the lines of a script by how completely the fan works quote them.

The script markup is written in lines, the `LINE<<...>>` tags; the other commands look at the
script by regions, scenes or characters and ask whether a work touches one.  This command takes
the line as its unit and measures: per line the works quoting it, whole, mostly (`--most`
percent of its words), from its first word, to its last word; per work the lines it quotes and
the one it quotes most of; per (line, work) cell the covered words, where they start and end and
in how many pieces.  A work covers every script word from the first record of one of its
passages to the last, bridged words included; a passage is what `passages` keeps under the same
`--min-words` and `--max-gap`.

Reading, sorting (passages.read_matches / sort_records), the line table of the markup and
writing are host plumbing; the passages, the coverage, the line x work incidence and the walk
over the cells come from the GPU (fs_lines).
"""

import ctypes as C

import numpy as np

from . import _lib, abi, vocab as vocab_mod
from .command import grow, prefixed, run, script_labels, work_names
from .passages import _ORIG_IX, _ORIG_WORD, sort_records
from .search import _CHAR_REX, _LINE_REX, _SCENE_REX

LINE_FIELDS = ['LINE', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'WORDS', 'CHARACTER', 'SCENE',
               'WORKS', 'WHOLE_WORKS', 'MOST_WORKS', 'HEAD_WORKS', 'TAIL_WORKS',
               'MEAN_SHARE_PERCENT', 'WHOLE_PERCENT', 'FIRST_FAN_WORK_FILENAME', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'LINES', 'WHOLE_LINES', 'COVERED_WORDS', 'LINE_WORDS',
               'SHARE_PERCENT', 'TOP_LINE', 'TOP_LINE_COVERED', 'TOP_LINE_WORDS', 'TOP_LINE_TEXT']
CELL_FIELDS = ['LINE', 'FAN_WORK_FILENAME', 'COVERED_WORDS', 'LINE_WORDS', 'SHARE_PERCENT',
               'FIRST_COVERED_WORD_INDEX', 'LAST_COVERED_WORD_INDEX', 'RUNS', 'WHOLE',
               'SPAN_TEXT']


def load_markup_lines(filename):
    """(rows, line_first) of a script markup: the rows [LOWERCASE, SPACY_ORTH_ID, SCENE,
    CHARACTER] under their header row exactly as search.load_markup_script gives them (the same
    regexes, first match wins per text line in the order scene / character / line, the same
    tokenizer), and the word index each line starts at, one entry per `LINE<<...>>` tag that
    yields a token, in file order, with the number of words behind them: line l owns the words
    line_first[l] .. line_first[l + 1] - 1 (word 0 is rows[1])."""
    rows = [['LOWERCASE', 'SPACY_ORTH_ID', 'SCENE', 'CHARACTER']]
    line_first = []
    scene = None
    scene_tags = 0
    count_scenes = False
    character = None
    with open(filename, encoding='utf-8') as ip:
        for text in ip:
            m = _SCENE_REX.search(text)
            if m:
                scene_tags += 1
                digits = ''.join(ch for ch in m.group('scene') if ch.isdigit())
                try:
                    scene = int(digits)
                except ValueError:      # (no digits: the running count of scene tags from here)
                    count_scenes = True
                if count_scenes:
                    scene = scene_tags
                continue
            m = _CHAR_REX.search(text)
            if m:
                character = m.group('character')
                continue
            m = _LINE_REX.search(text)
            if m:
                at = len(rows) - 1
                for tok in vocab_mod.tokenize(m.group('line')):
                    low = tok.lower()
                    rows.append([low, vocab_mod.hash_string(low), scene, character])
                if len(rows) - 1 > at:
                    line_first.append(at)
    line_first.append(len(rows) - 1)
    return rows, line_first


def find_lines(work, fan_ix, orig_ix, n_works, n_script, line_first, min_words=6, max_gap=0,
               most=50, device=0):
    """(abi.LINE_DTYPE[n_lines], abi.LINE_WORK_DTYPE per active work, abi.LINE_CELL_DTYPE cells
    in (line, work) order) of records sorted by (work, fan_ix) and the line table
    line_first[n_lines + 1] over the n_script words."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    line_first = abi.as_u32(line_first)
    n = len(work)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(line_first) < 1:
        raise ValueError("a line table holds at least the number of script words")
    n_lines = len(line_first) - 1
    L = _lib.load()
    lines = np.zeros(n_lines, dtype=abi.LINE_DTYPE)
    works, cells = grow(lambda w_out, w_cap, w_got, c_out, c_cap, c_got: L.fs_lines(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script),
        abi.ptr(line_first, C.c_uint32), n_lines, int(min_words), int(max_gap), int(most),
        lines.ctypes.data_as(C.c_void_p), w_out, w_cap, w_got, c_out, c_cap, c_got),
        [abi.LINE_WORK_DTYPE, abi.LINE_CELL_DTYPE], [256, 4096], "fs_lines")
    return lines, works, cells


def check_records(orig, word_at, markup_rows):
    """ValueError for records that were not searched against this markup: a script word index at
    or beyond its word count, or an ORIGINAL_SCRIPT_WORD (the markup's LOWERCASE, as `search`
    writes it) that differs from the markup's word at its index.  `word_at`: {script word index:
    the word its records carry}."""
    n_script = len(markup_rows) - 1
    if len(orig) and int(orig.max()) >= n_script:
        far = int(orig.max())
        raise ValueError("ORIGINAL_SCRIPT_WORD_INDEX %d in a script markup of %d words (the "
                         "records need at least %d): was the file searched against another "
                         "script?" % (far, n_script, far + 1))
    for o in sorted(word_at):
        if word_at[o] != markup_rows[o + 1][0]:
            raise ValueError("script word %d is %r in the records and %r in the script markup: "
                             "was the file searched against another script?"
                             % (o, word_at[o], markup_rows[o + 1][0]))


def tables(rows, markup, min_words=6, max_gap=0, min_works=1, most=50, device=0):
    """(lines, works, cells): the three CSVs' rows, without headers, for the records `rows`
    (read_matches) and the markup (load_markup_lines)."""
    _, work, fan, orig, _, _ = sort_records(rows)
    n_script = len(markup[0]) - 1
    word_at = {}
    for r in rows:            # per script word its first record that differs from the markup
        o, word = int(r[_ORIG_IX]), r[_ORIG_WORD]
        if o not in word_at or (o < n_script and word_at[o] == markup[0][o + 1][0] != word):
            word_at[o] = word
    check_records(orig, word_at, markup[0])
    return _tables(work_names(rows), work, fan, orig, markup, min_words, max_gap, min_works,
                   most, device)


def tables_device(mf, markup, min_words=6, max_gap=0, min_works=1, most=50, device=0):
    """tables over a matches.MatchFile; None when a script word's records spell a label in two
    ways (tables() then says what is wrong)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = len(markup[0]) - 1
    check_records(orig, {}, markup[0])              # (the labels are read per script word)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    check_records(orig, {o: lab[0] for o, lab in labels.items()}, markup[0])
    return _tables(list(mf.names), work, fan, orig, markup, min_words, max_gap, min_works, most,
                   device)


def _tables(names, work, fan, orig, markup, min_words, max_gap, min_works, most, device):
    if not 1 <= most <= 100:
        raise ValueError("--most %d: a whole percentage from 1 to 100" % most)
    if min_words < 1:
        raise ValueError("--min-words must be at least 1")
    rows, line_first = markup
    n_script = len(rows) - 1
    lines, works, cells = find_lines(work, fan, orig, len(names), n_script, line_first,
                                     min_words, max_gap, most, device)

    def text(a, b):
        return ' '.join(rows[o + 1][0] for o in range(a, b + 1))

    def words(l):
        return line_first[l + 1] - line_first[l]
    # WORKS descending, then WHOLE_WORKS descending, then the line: one key, a stable sort
    key = (lines['works'].astype(np.int64) << 32) | lines['whole_works'].astype(np.int64)
    keep = np.flatnonzero(lines['works'] >= max(int(min_works), 0))
    keep = keep[np.argsort(-key[keep], kind='stable')]
    ltab = []
    for l in keep.tolist():
        v = lines[l]
        a, b, n, k = line_first[l], line_first[l + 1] - 1, int(v['works']), words(l)
        first = int(v['first_work'])
        ltab.append([l + 1, a, b, k, rows[a + 1][3], rows[a + 1][2], n, int(v['whole_works']),
                     int(v['most_works']), int(v['head_works']), int(v['tail_works']),
                     int(v['covered_sum']) * 100 // (n * k) if n else 0,
                     int(v['whole_works']) * 100 // n if n else 0,
                     '' if first == abi.FS_NONE else names[first], text(a, b)])
    wtab = []
    for v in works:
        top = int(v['top_line'])
        wtab.append([names[int(v['work'])], int(v['lines']), int(v['whole_lines']),
                     int(v['covered']), int(v['line_words']),
                     int(v['covered']) * 100 // int(v['line_words']), top + 1,
                     int(v['top_covered']), words(top),
                     text(line_first[top], line_first[top + 1] - 1)])
    ctab = []
    for v in cells:
        l, n, k = int(v['line']), int(v['covered']), words(int(v['line']))
        ctab.append([l + 1, names[int(v['work'])], n, k, n * 100 // k, int(v['first']),
                     int(v['last']), int(v['runs']), 1 if n == k else 0,
                     text(int(v['first']), int(v['last']))])
    return ltab, wtab, ctab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-lines.csv', '-lines-works.csv', '-lines-cells.csv'))


def process(args):
    """`ao3.py lines matches script [-o PREFIX] [--min-words M] [--max-gap G] [--min-works K]
    [--most P] [--device D] [--reader {device,python}]`."""
    markup = load_markup_lines(args.script)
    opts = (markup, args.min_words, args.max_gap, args.min_works, args.most, args.device)
    return run(args, (LINE_FIELDS, WORK_FIELDS, CELL_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
