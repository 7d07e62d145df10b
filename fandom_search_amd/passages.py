"""`ao3.py passages`: the per-word match records of a search joined into passages of reuse.

`search` writes one record per matched fan word.  A passage is a run of records of one fan
work whose fan and script indices both step forward together (by 1, or by up to 1 + G with
`--max-gap G`, so that a passage bridges G words without a record); runs of at least
`--min-words` records are kept.  Unlike `matrix`, which keeps one most-common n-gram per span
and counts it per work, every passage is listed with its location on both sides, its words
and its distances.

The records are sorted stably by (work, FAN_WORK_WORD_INDEX) on the host, work being the
first-appearance order of FAN_WORK_FILENAME (as in `matrix`); the join and the sums and
maxima run on the GPU (fs_passages); reading and writing the CSV is host plumbing.
"""

import csv
import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, write_tables
from .search import new_record_structure

FIELDS = new_record_structure['fields']
(_FNAME, _FAN_IX, _FAN_WORD, _, _ORIG_IX, _ORIG_WORD, _, _CHAR, _SCENE, _DIST, _,
 _COMB) = range(len(FIELDS))

PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                  'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                  'EXACT_WORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE',
                  'MEAN_MATCH_DISTANCE', 'MAX_MATCH_DISTANCE', 'MEAN_COMBINED_DISTANCE',
                  'MAX_COMBINED_DISTANCE', 'FAN_WORK_TEXT', 'ORIGINAL_SCRIPT_TEXT']


def find_passages(work, fan_ix, orig_ix, dist, comb, min_words=6, max_gap=0, device=0):
    """Passages (abi.PASSAGE_DTYPE, host) of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    comb = np.ascontiguousarray(comb, dtype=np.float64)
    n = len(work)
    if not (len(fan) == len(orig) == len(dist) == len(comb) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    cap = n // max(1, int(min_words)) + 1          # passages never outnumber this
    return grow(lambda out, cap, got: L.fs_passages(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(dist, C.c_double), abi.ptr(comb, C.c_double), n,
        int(min_words), int(max_gap), out, cap, got), abi.PASSAGE_DTYPE, cap, "fs_passages")


def _distance(text):
    return float(text) if text else float('nan')


def read_matches(path):
    """The records of a match CSV (a dated file with its header row, or a batch file
    without), as text rows in file order."""
    with open(path, newline='', encoding='utf-8') as fh:
        rows = [r for r in csv.reader(fh) if r]
    if rows and rows[0] == FIELDS:
        rows = rows[1:]
    return rows


def sort_records(rows):
    """(order, work, fan_ix, orig_ix, dist, comb): the stable (work, fan_ix) order of the
    records and their numeric columns in that order."""
    work_of = {}
    work = np.fromiter((work_of.setdefault(r[_FNAME], len(work_of)) for r in rows),
                       dtype=np.int64, count=len(rows))
    fan = np.fromiter((int(r[_FAN_IX]) for r in rows), dtype=np.int64, count=len(rows))
    orig = np.fromiter((int(r[_ORIG_IX]) for r in rows), dtype=np.int64, count=len(rows))
    if len(rows) and (min(fan.min(), orig.min()) < 0 or max(fan.max(), orig.max()) >= 1 << 32):
        raise ValueError("word indices outside 0 .. 2^32 - 1")
    dist = np.fromiter((_distance(r[_DIST]) for r in rows), dtype=np.float64, count=len(rows))
    comb = np.fromiter((_distance(r[_COMB]) for r in rows), dtype=np.float64, count=len(rows))
    order = np.lexsort((fan, work))
    return order, work[order], fan[order], orig[order], dist[order], comb[order]


def passage_rows(rows, min_words=6, max_gap=0, device=0):
    """The passage CSV's rows (without header) for the records `rows` (read_matches)."""
    order, work, fan, orig, dist, comb = sort_records(rows)
    found = find_passages(work, fan, orig, dist, comb, min_words, max_gap, device)
    out = []
    for p in found:
        a, k = int(p['first']), int(p['n_words'])
        recs = [rows[i] for i in order[a:a + k]]
        head = recs[0]
        out.append([head[_FNAME], int(fan[a]), int(fan[a + k - 1]), int(orig[a]),
                    int(orig[a + k - 1]), k, int(p['n_exact']), head[_CHAR], head[_SCENE],
                    float(p['dist_sum']) / k, float(p['dist_max']),
                    float(p['comb_sum']) / k, float(p['comb_max']),
                    ' '.join(r[_FAN_WORD] for r in recs),
                    ' '.join(r[_ORIG_WORD] for r in recs)])
    return out


def passage_rows_device(mf, min_words=6, max_gap=0, device=0):
    """passage_rows over a matches.MatchFile: the same rows, decoding only the fields of the
    records inside passages."""
    order, work, fan, orig, dist, comb = mf.sorted()
    found = find_passages(work, fan, orig, dist, comb, min_words, max_gap, device)
    first = found['first'].astype(np.int64)
    count = found['n_words'].astype(np.int64)
    ends = np.cumsum(count)
    # the records of every kept passage, passage after passage
    pos = np.repeat(first - (ends - count), count) + np.arange(ends[-1] if len(ends) else 0)
    recs = order[pos]
    fan_words, orig_words = mf.text(_FAN_WORD, recs), mf.text(_ORIG_WORD, recs)
    heads = order[first]
    names, chars, scenes = (mf.text(c, heads) for c in (_FNAME, _CHAR, _SCENE))
    out = []
    for j, p in enumerate(found):
        a, k = int(p['first']), int(p['n_words'])
        lo, hi = int(ends[j]) - k, int(ends[j])
        out.append([names[j], int(fan[a]), int(fan[a + k - 1]), int(orig[a]),
                    int(orig[a + k - 1]), k, int(p['n_exact']), chars[j], scenes[j],
                    float(p['dist_sum']) / k, float(p['dist_max']),
                    float(p['comb_sum']) / k, float(p['comb_max']),
                    ' '.join(fan_words[lo:hi]), ' '.join(orig_words[lo:hi])])
    return out


def body_rows(path, reader, min_words=6, max_gap=0, device=0):
    """The passage CSV's rows of the match file `path` under `reader` ('device' or 'python');
    a file the device reader does not take goes through read_matches like any file did."""
    if reader == 'device':
        from .matches import MatchFile
        with MatchFile(path, device) as mf:
            if not mf.outside:
                return passage_rows_device(mf, min_words, max_gap, device)
    return passage_rows(read_matches(path), min_words, max_gap, device)


def output_name(matches):
    return (matches[:-4] if matches.endswith('.csv') else matches) + '-passages.csv'


def process(args):
    """`ao3.py passages matches [-o OUTPUT] [--min-words M] [--max-gap G] [--device D]
    [--reader {device,python}]`."""
    from .matches import reader_of
    out = args.output or output_name(args.matches)
    body = body_rows(args.matches, reader_of(args), args.min_words, args.max_gap, args.device)
    write_tables([out], [PASSAGE_FIELDS], [body])
    return out
