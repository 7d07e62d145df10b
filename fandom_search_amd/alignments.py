"""`ao3.py alignments`: quotes with inserted or dropped words.

`passages` joins a record to the record directly behind it, and only when both indices step
forward together; a fan who inserts a word that found a stray match elsewhere, or drops one,
breaks the passage in two, and both halves may fall under `--min-words`.  This command aligns
every fan work against the script with gaps instead.  Record j may precede record i of the same
work when the fan and the script index each step 1 .. 1 + `--reach` ahead, whatever lies between
them; the link costs `--gap` per word skipped on either side, a record scores `--match`, and

    best(i) = match + max(0, max over such j of best(j) - cost(j, i)).

The records linked to one root form a tree; its alignment is the path from the root to the
record with the largest best, and paths of at least `--min-words` records are listed.

The records are sorted by (work, FAN_WORK_WORD_INDEX) as `passages` sorts them.  The recurrence,
the figures of every alignment and the list of its records come from the GPU (fs_alignments);
the two distance columns, the per-work sums (np.bincount over the alignment records), reading
labels and writing the CSVs is host plumbing, and only the fields of records on kept paths are
decoded to text.
"""

import ctypes as C
import math

import numpy as np

from . import _lib, abi
from .command import grow, prefixed, run, work_names
from .passages import _CHAR, _FAN_WORD, _ORIG_WORD, _SCENE, find_passages, sort_records

ALIGNMENT_FIELDS = ['FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                    'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                    'EXACT_WORDS', 'SCORE', 'FAN_WORDS_SKIPPED', 'SCRIPT_WORDS_SKIPPED', 'PIECES',
                    'SIDE_RECORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE',
                    'MEAN_COMBINED_DISTANCE', 'MAX_COMBINED_DISTANCE', 'FAN_WORK_TEXT',
                    'ORIGINAL_SCRIPT_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'ALIGNMENTS', 'ALIGNED_WORDS', 'LONGEST', 'FAN_WORDS_SKIPPED',
               'SCRIPT_WORDS_SKIPPED', 'PASSAGE_WORDS', 'GAINED_WORDS']


def find_alignments(work, fan_ix, orig_ix, comb, min_words=6, reach=4, match=2, gap=1, device=0):
    """(abi.ALIGNMENT_DTYPE alignments in root order, uint32 record indices of their paths, path
    after path) of records sorted by (work, fan_ix)."""
    work, fan, orig = (abi.as_u32(v) for v in (work, fan_ix, orig_ix))
    comb = np.ascontiguousarray(comb, dtype=np.float64)
    n = len(work)
    if not (len(fan) == len(orig) == len(comb) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    return grow(lambda out, cap, got, path, path_cap, path_got: L.fs_alignments(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(comb, C.c_double), n, int(min_words), int(reach),
        int(match), int(gap), out, cap, got, path, path_cap, path_got),
        [abi.ALIGNMENT_DTYPE, np.uint32], [min(n // max(1, int(min_words)), 4096), min(n, 1 << 16)],
        "fs_alignments")


def tables(rows, min_words=6, reach=4, match=2, gap=1, device=0):
    """(alignments, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    def field(column, recs):
        return [rows[i][column] for i in recs]
    return _tables(work_names(rows), field, sort_records(rows), min_words, reach, match, gap,
                   device)


def tables_device(mf, min_words=6, reach=4, match=2, gap=1, device=0):
    """tables over a matches.MatchFile, decoding only the fields of the records on kept paths."""
    return _tables(mf.names, mf.text, mf.sorted(), min_words, reach, match, gap, device)


def _max(values):
    """The largest value that is not NaN, the earlier one on a tie; NaN without one."""
    best = float('nan')
    for v in values:
        if not math.isnan(v) and (math.isnan(best) or v > best):
            best = v
    return best


def _text(words, skips):
    """The words joined by a space, [+k] where the link between two of them skips k words."""
    out = [words[0]]
    for word, k in zip(words[1:], skips):
        if k:
            out.append('[+%d]' % k)
        out.append(word)
    return ' '.join(out)


def _tables(names, field, columns, min_words, reach, match, gap, device):
    order, work, fan, orig, dist, comb = columns
    found, path = find_alignments(work, fan, orig, comb, min_words, reach, match, gap, device)
    path = path.astype(np.int64)
    recs = order[path]
    fans, origs = field(_FAN_WORD, recs), field(_ORIG_WORD, recs)
    heads = order[found['first'].astype(np.int64)]
    chars, scenes = field(_CHAR, heads), field(_SCENE, heads)
    pfan, porig = fan[path].tolist(), orig[path].tolist()
    pcomb = comb[path].tolist()
    atab = []
    for k, a in enumerate(found):
        lo = int(a['path_at'])
        hi = lo + int(a['n_words'])
        f, o, c = pfan[lo:hi], porig[lo:hi], pcomb[lo:hi]
        atab.append([names[int(work[int(a['first'])])], f[0], f[-1], o[0], o[-1],
                     int(a['n_words']), int(a['n_exact']), int(a['score']),
                     int(a['fan_skipped']), int(a['orig_skipped']), int(a['pieces']),
                     int(a['tree_records']) - int(a['n_words']), chars[k], scenes[k],
                     sum(c, 0.0) / len(c), _max(c),
                     _text(fans[lo:hi], [y - x - 1 for x, y in zip(f, f[1:])]),
                     _text(origs[lo:hi], [y - x - 1 for x, y in zip(o, o[1:])])])
    # per work: sums over the alignment records, and the words `passages` joins under the same M
    n_works = len(names)
    mine = work[found['first'].astype(np.int64)].astype(np.int64)

    def per_work(values):
        return np.bincount(mine, weights=values, minlength=n_works).astype(np.int64)
    count = np.bincount(mine, minlength=n_works)
    words = per_work(found['n_words'])
    longest = np.zeros(n_works, dtype=np.int64)
    np.maximum.at(longest, mine, found['n_words'].astype(np.int64))
    fsk, osk = per_work(found['fan_skipped']), per_work(found['orig_skipped'])
    joined = find_passages(work, fan, orig, dist, comb, min_words, 0, device)
    inside = np.bincount(work[joined['first'].astype(np.int64)].astype(np.int64),
                         weights=joined['n_words'], minlength=n_works).astype(np.int64)
    wtab = [[names[w], int(count[w]), int(words[w]), int(longest[w]), int(fsk[w]), int(osk[w]),
             int(inside[w]), int(words[w] - inside[w])] for w in np.flatnonzero(count).tolist()]
    return atab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-alignments.csv', '-alignments-works.csv'))


def process(args):
    """`ao3.py alignments matches [-o PREFIX] [--min-words M] [--reach R] [--match S] [--gap P]
    [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.reach, args.match, args.gap, args.device)
    return run(args, (ALIGNMENT_FIELDS, WORK_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
