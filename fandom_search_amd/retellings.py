"""`ao3.py retellings`: fan works that quote the script in the script's own order.

`works` says how much a fan work quotes and from where; this command says in what order.  The
passages of a work (as `passages` joins them) are numbered in record order, that is in the order
the work has them.  A passage may follow an earlier one when it starts after the script word the
earlier one ends at; the work's chain is the heaviest sequence of passages each following the one
before, by matched words.  A retelling that walks through the film scene after scene has nearly
all its passage words in its chain; a work that quotes the same lines shuffled has few.

The records are sorted by (work, FAN_WORK_WORD_INDEX) as `passages` sorts them.  The passages,
the chain of every work (a dynamic programme per work), its descents and the place of every
passage in the chain come from the GPU (fs_retellings); choosing and ordering the listed works
(a stable sort of at most one key per work), reading labels and writing the CSVs is host
plumbing, and only the fields the listed rows show are decoded to text.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, work_names
from .passages import _CHAR, _FAN_WORD, _ORIG_WORD, _SCENE, sort_records
from .quotes import word_labels

WORK_FIELDS = ['FAN_WORK_FILENAME', 'PASSAGES', 'PASSAGE_WORDS', 'CHAIN_PASSAGES', 'CHAIN_WORDS',
               'IN_ORDER_PERCENT', 'DESCENTS', 'ORIGINAL_SCRIPT_WORD_INDEX',
               'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'SCRIPT_SPAN_WORDS', 'CHAIN_SCRIPT_WORDS',
               'FAN_WORK_WORD_INDEX', 'LAST_FAN_WORK_WORD_INDEX', 'SCENES', 'SCENE_SEQUENCE']
PASSAGE_FIELDS = ['FAN_WORK_FILENAME', 'PASSAGE', 'FAN_WORK_WORD_INDEX',
                  'LAST_FAN_WORK_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD_INDEX',
                  'LAST_ORIGINAL_SCRIPT_WORD_INDEX', 'WORDS', 'ORIGINAL_SCRIPT_CHARACTER',
                  'ORIGINAL_SCRIPT_SCENE', 'IN_CHAIN', 'CHAIN_POSITION', 'FAN_TEXT', 'SCRIPT_TEXT']


def find_retellings(work, fan_ix, orig_ix, n_works, min_words=6, max_gap=0, device=0):
    """(abi.RETELLING_DTYPE[n_works], abi.RETELLING_PASSAGE_DTYPE passages in record order) of
    records sorted by (work, fan_ix)."""
    work, fan, orig = (abi.as_u32(v) for v in (work, fan_ix, orig_ix))
    n = len(work)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    out = np.empty(int(n_works), dtype=abi.RETELLING_DTYPE)
    found = grow(lambda found, cap, got: L.fs_retellings(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(min_words), int(max_gap),
        out.ctypes.data_as(C.c_void_p), found, cap, got),
        abi.RETELLING_PASSAGE_DTYPE, min(n // max(1, int(min_words)), 4096), "fs_retellings")
    return out, found


def tables(rows, min_words=6, max_gap=0, min_passages=2, min_share=0, device=0):
    """(works, passages): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    word_labels(rows)                   # a script word with two labels is an error
    order, work, fan, orig, _, _ = sort_records(rows)

    def field(column, recs):
        return [rows[i][column] for i in recs]
    return _tables(work_names(rows), field, order, work, fan, orig, min_words, max_gap, min_passages,
                   min_share, device)


def tables_device(mf, min_words=6, max_gap=0, min_passages=2, min_share=0, device=0):
    """tables over a matches.MatchFile, decoding only the fields of the listed works' passages;
    None when a script word's records spell a label in two ways (tables() then decides)."""
    order, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    for column in (_ORIG_WORD, _CHAR, _SCENE) if mf.n else ():
        if mf.label_rows(column, n_script)[1]:
            return None
    return _tables(mf.names, mf.text, order, work, fan, orig, min_words, max_gap, min_passages,
                   min_share, device)


def _tables(names, field, order, work, fan, orig, min_words, max_gap, min_passages, min_share,
            device):
    works, found = find_retellings(work, fan, orig, len(names), min_words, max_gap, device)
    share = works['chain_words'].astype(np.int64) * 100 // np.maximum(works['passage_words'], 1)
    keep = np.flatnonzero((works['n_passages'] > 0) & (works['chain_passages'] >= min_passages)
                          & (share >= min_share))
    # CHAIN_WORDS descending, then CHAIN_PASSAGES descending, then first appearance
    keep = keep[np.lexsort((keep, -works['chain_passages'][keep].astype(np.int64),
                            -works['chain_words'][keep].astype(np.int64)))]
    start = np.searchsorted(found['work'], keep, side='left')
    # the listed works' passages, work after work
    count = works['n_passages'][keep].astype(np.int64)
    ends = np.cumsum(count)
    which = np.repeat(start - (ends - count), count) + np.arange(ends[-1] if len(ends) else 0)
    mine = found[which]
    first = mine['first'].astype(np.int64)
    words = mine['n_words'].astype(np.int64)
    wends = np.cumsum(words)
    pos = np.repeat(first - (wends - words), words) + np.arange(wends[-1] if len(wends) else 0)
    recs = order[pos]
    fans, origs = field(_FAN_WORD, recs), field(_ORIG_WORD, recs)
    heads = order[first]
    chars, scenes = field(_CHAR, heads), field(_SCENE, heads)
    wtab, ptab = [], []
    for k, w in enumerate(keep.tolist()):
        r, name = works[w], names[w]
        lo, hi = int(ends[k] - count[k]), int(ends[k])
        chain = sorted((int(mine[j]['chain_pos']), j) for j in range(lo, hi)
                       if mine[j]['chain_pos'])
        seq = [scenes[j] for _, j in chain]
        seq = [s for i, s in enumerate(seq) if i == 0 or seq[i - 1] != s]
        a, b = int(r['orig_first']), int(r['orig_last'])
        wtab.append([name, int(r['n_passages']), int(r['passage_words']),
                     int(r['chain_passages']), int(r['chain_words']), int(share[w]),
                     int(r['n_descents']), a, b, b - a + 1, int(r['chain_script_words']),
                     int(found[int(r['chain_first'])]['fan_first']),
                     int(found[int(r['chain_last'])]['fan_last']),
                     len(set(scenes[j] for _, j in chain)), ' > '.join(seq)])
        for j in range(lo, hi):
            p = mine[j]
            t0, t1 = int(wends[j] - words[j]), int(wends[j])
            at = int(p['chain_pos'])
            ptab.append([name, j - lo + 1, int(p['fan_first']), int(p['fan_last']),
                         int(p['orig_first']), int(p['orig_last']), int(p['n_words']), chars[j],
                         scenes[j], 1 if at else 0, at if at else '', ' '.join(fans[t0:t1]),
                         ' '.join(origs[t0:t1])])
    return wtab, ptab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-retellings.csv', '-retellings-passages.csv'))


def process(args):
    """`ao3.py retellings matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-passages P]
    [--min-share S] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.min_passages, args.min_share, args.device)
    return run(args, (WORK_FIELDS, PASSAGE_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
