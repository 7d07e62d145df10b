"""`ao3.py matrix`: works x phrases count matrix from a match CSV.

The reference advertises this command (README.md:74,149-160) but its code is
an orphan (/root/reference/_deprecated.py:83-89 subparser, :91-302
StrictNgramDedupe, :305-316 process): never imported, and `process` indexes an
argparse Namespace like a dict, so it cannot run.  This module implements the
evident intent of that code:

  1. group match rows by fan work (first-appearance order)        (:97-101)
  2. per work: runs of consecutive FAN_WORK_WORD_INDEX, inside each run the
     runs of consecutive ORIGINAL_SCRIPT_WORD_INDEX, keeping runs of at least n
     rows -- contiguous verbatim spans                            (:251-277)
  3. count, over all works, every n-gram start inside those spans, keyed by
     script word index                                            (:104-108, :279-282)
  4. per span keep the n-gram whose start is most common (first maximum)
                                                                  (:297-302)
  5. drop it when some start within +-(n-1) script words is more common (first
     maximum over ascending start positions must be the n-gram itself)
                                                                  (:290-295)
  6. matrix: one column per phrase (lower-cased script words joined by spaces)
     ordered by script index, a '(total)' row, one row per work sorted by file
     name; file '<m>-most-common-perfect-matches-no-overlap-<n>-gram-match-
     matrix.csv'                                                  (:124-149, :310)
"""

import collections
import csv


def _runs(rows, key):
    """Stable sort by int(row[key]) and split where the key is not previous+1."""
    rows = sorted(rows, key=lambda r: int(r[key]))
    out, cur, prev = [], [], None
    for r in rows:
        val = int(r[key])
        if cur and val != prev + 1:
            out.append(cur)
            cur = []
        cur.append(r)
        prev = val
    if cur:
        out.append(cur)
    return out


class StrictNgramDedupe(object):
    def __init__(self, data_path, ngram_size):
        self.ngram_size = n = int(ngram_size)
        with open(data_path, encoding='UTF8') as ip:
            self.data = list(csv.DictReader(ip))
        self.work_matches = collections.OrderedDict()
        for r in self.data:
            self.work_matches.setdefault(r['FAN_WORK_FILENAME'], []).append(r)

        spans = [span for rows in self.work_matches.values()
                 for span in self.segment_full(rows)]
        self.starts_counter = collections.Counter(
            int(span[i]['ORIGINAL_SCRIPT_WORD_INDEX'])
            for span in spans for i in range(len(span) - n + 1))
        picked = [self.top_ngram(span) for span in spans]
        self.filtered_matches = [ng for ng in picked if self.no_better_match(ng)]

    def segment_full(self, rows):
        n = self.ngram_size
        return [orig_run
                for fan_run in _runs(rows, 'FAN_WORK_WORD_INDEX')
                for orig_run in _runs(fan_run, 'ORIGINAL_SCRIPT_WORD_INDEX')
                if len(orig_run) >= n]

    def top_ngram(self, span):
        n = self.ngram_size
        count = self.starts_counter
        start = max(range(len(span) - n + 1),
                    key=lambda i: count[int(span[i]['ORIGINAL_SCRIPT_WORD_INDEX'])])
        return span[start:start + n]

    def no_better_match(self, ng):
        n = self.ngram_size
        start = int(ng[0]['ORIGINAL_SCRIPT_WORD_INDEX'])
        best = max(range(start - n + 1, start + n),
                   key=lambda s: self.starts_counter[s])
        return best == start

    def num_ngrams(self):
        return len(set(int(ng[0]['ORIGINAL_SCRIPT_WORD_INDEX'])
                       for ng in self.filtered_matches))

    @staticmethod
    def match_to_phrase(match):
        return ' '.join(m['ORIGINAL_SCRIPT_WORD'].lower() for m in match)

    def matrix_rows(self):
        return self.tables()[0]

    def tables(self):
        """(the matrix's rows, the start each phrase's column ended up with)."""
        phrase_ix = {}
        works = set()
        cells = collections.defaultdict(int)
        for m in self.filtered_matches:
            phrase = self.match_to_phrase(m)
            phrase_ix[phrase] = int(m[0]['ORIGINAL_SCRIPT_WORD_INDEX'])
            works.add(m[0]['FAN_WORK_FILENAME'])
            cells[(m[0]['FAN_WORK_FILENAME'], phrase)] += 1
        phrases = sorted(phrase_ix, key=phrase_ix.get)
        works = sorted(works)
        body = [[cells[(fn, ph)] for ph in phrases] for fn in works]
        totals = [sum(col) for col in zip(*body)] if body else []
        return ([['FILENAME'] + phrases, ['(total)'] + totals]
                + [[fn] + r for fn, r in zip(works, body)]), [phrase_ix[ph] for ph in phrases]

    def write_match_work_count_matrix(self, out_filename):
        write_rows(out_filename, self.matrix_rows())


def write_rows(out_filename, rows):
    with open(out_filename, 'w', encoding='utf-8') as op:
        csv.writer(op).writerows(rows)


CELL_FIELDS = ['FILENAME', 'PHRASE_INDEX', 'ORIGINAL_SCRIPT_WORD_INDEX', 'PHRASE', 'COUNT']


def cell_rows(rows, starts):
    """The non-zero cells of the matrix `rows` (its '(total)' row included, as the first rows:
    the list of the phrases), in row order then column order; PHRASE_INDEX is the 1-based
    column and starts[column - 1] the script index the column stands at."""
    phrases = rows[0][1:]
    out = [CELL_FIELDS]
    for row in rows[1:]:
        out.extend([row[0], k + 1, starts[k], phrases[k], c]
                   for k, c in enumerate(row[1:]) if c)
    return out


def device_tables(data_path, ngram_size, device=0):
    """StrictNgramDedupe(data_path, ngram_size).tables() with steps 1-5 on HIP device `device`,
    or None for a file the Python engine has to take: one outside the device reader's grammar
    or without the header row, a script word spelt in two ways, a '\r' in a text this command
    shows (StrictNgramDedupe reads with universal newlines, which turn it into '\n'), or more
    than fs_matrix supports."""
    import numpy as np

    from . import _lib, abi
    from .command import n_script_of
    from .matches import MatchFile
    from .passages import _ORIG_WORD
    n = int(ngram_size)
    with MatchFile(data_path, device) as mf:
        if mf.outside or not mf.has_header or any('\r' in name for name in mf.names):
            return None
        _, work, fan, orig, _, _ = mf.sorted()
        n_script = n_script_of(orig)
        try:
            kept = find_ngrams(work, fan, orig, len(mf.names), n_script, n, device)[2]
        except _lib.FsError as e:
            if e.code == abi.FS_E_UNSUPPORTED:
                return None
            raise
        if not len(kept):
            return [['FILENAME'], ['(total)']], []
        label = mf.labels(_ORIG_WORD, n_script)
        if label is None or any('\r' in text for text in label.values()):
            return None
        names = mf.names
    start = kept['start'].astype(np.int64)
    # a phrase stands at the start of its last n-gram in span order
    uniq, inv = np.unique(start, return_inverse=True)
    last = np.zeros(len(uniq), dtype=np.int64)
    last[inv] = np.arange(len(start))
    phrase_ix, seen_at = {}, {}
    text = [' '.join(label[s + k].lower() for k in range(n)) for s in uniq.tolist()]
    for s, at, phrase in zip(uniq.tolist(), last.tolist(), text):
        if seen_at.get(phrase, -1) < at:
            seen_at[phrase], phrase_ix[phrase] = at, s
    phrases = sorted(phrase_ix, key=phrase_ix.get)
    column = {phrase: k for k, phrase in enumerate(phrases)}
    col = np.array([column[phrase] for phrase in text], dtype=np.int64)[inv]
    # the works by file name, their cells by column
    works = np.array(sorted(np.unique(kept['work']).tolist(), key=names.__getitem__),
                     dtype=np.int64)
    row_of = np.zeros(len(names), dtype=np.int64)
    row_of[works] = np.arange(len(works))
    cell, count = np.unique(row_of[kept['work']] * len(phrases) + col, return_counts=True)
    totals = np.bincount(col, minlength=len(phrases)).tolist()
    body = [[0] * len(phrases) for _ in range(len(works))]
    for at, c in zip(cell.tolist(), count.tolist()):
        body[at // len(phrases)][at % len(phrases)] = c
    rows = ([['FILENAME'] + phrases, ['(total)'] + totals]
            + [[names[w]] + r for w, r in zip(works.tolist(), body)])
    return rows, [phrase_ix[ph] for ph in phrases]


def find_ngrams(work, fan_ix, orig_ix, n_works, n_script, ngram, device=0):
    """(starts[n_script], n_spans, abi.MATRIX_NGRAM_DTYPE kept n-grams in span order) of records
    sorted by (work, fan_ix): fs_matrix."""
    import ctypes as C

    import numpy as np

    from . import _lib, abi
    from .command import grow
    work, fan, orig = (abi.as_u32(v) for v in (work, fan_ix, orig_ix))
    n = len(work)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    starts = np.zeros(int(n_script), dtype=np.uint32)
    spans = C.c_uint64(0)
    found = grow(lambda found, cap, got: L.fs_matrix(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), int(ngram),
        abi.ptr(starts, C.c_uint32), found, cap, C.byref(spans), got),
        abi.MATRIX_NGRAM_DTYPE, min(n // max(1, int(ngram)) + 1, 4096), "fs_matrix")
    return starts, int(spans.value), found


def matrix_filename(prefix, ngram_size):
    return ('{}-most-common-perfect-matches-no-overlap-{}-gram-match-matrix.csv'
            .format(prefix, ngram_size))


def cells_filename(prefix, ngram_size):
    return ('{}-most-common-perfect-matches-no-overlap-{}-gram-match-cells.csv'
            .format(prefix, ngram_size))


def process(args):
    """`ao3.py matrix i m [-n N] [--engine {python,device}] [--device D] [--cells]`."""
    tables = None
    if getattr(args, 'engine', 'python') == 'device' and int(args.n) >= 1:
        tables = device_tables(args.i, args.n, getattr(args, 'device', 0))
    if tables is None:          # the python engine, or a file the device engine does not take
        tables = StrictNgramDedupe(args.i, ngram_size=args.n).tables()
    out = matrix_filename(args.m, int(args.n))
    write_rows(out, tables[0])
    if getattr(args, 'cells', False):
        write_rows(cells_filename(args.m, int(args.n)), cell_rows(*tables))
    return out
