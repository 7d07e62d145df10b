"""`ao3.py quotes`: the per-word match records of a search seen from the script's side.

`format` counts records per script word, `passages` lists every reused span of every fan work,
`works` reduces the records by fan work.  This command answers which stretches of the script
fans quote and how many different works quote each one: per script word the distinct works
behind its records and behind the passages covering it (its depth), and the regions, maximal
stretches of depth >= `--min-works`, ranked material for a reader: their passages, works,
matched words and the peak of the depth with where it lies.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the distinct counts and the regions come from the GPU (fs_quotes).  A passage is what
`passages` keeps under the same `--min-words` and `--max-gap`; it covers every script word
between its first and last record, bridged ones included.
"""

import csv
import ctypes as C

import numpy as np

from . import _lib, abi
from .passages import (_CHAR, _FNAME, _ORIG_IX, _ORIG_WORD, _SCENE, read_matches,
                       sort_records)

REGION_FIELDS = ['ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'WORDS',
                 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'PASSAGES', 'WORKS',
                 'MATCHED_WORDS', 'EXACT_WORDS', 'PEAK_WORKS', 'PEAK_WORD_START',
                 'PEAK_WORD_END', 'ORIGINAL_SCRIPT_TEXT']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'MATCHED_WORDS',
               'EXACT_WORDS', 'WORKS', 'PASSAGES', 'PASSAGE_WORKS', 'REGION']
UNKNOWN_WORD = '[?]'       # a bridged script word no record names (no single token looks so)


def find_quotes(work, fan_ix, orig_ix, comb, n_works, n_script, min_words=6, max_gap=0,
                min_works=1, device=0):
    """(abi.QUOTE_WORD_DTYPE[n_script], abi.QUOTE_REGION_DTYPE regions in script order) of
    records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    comb = np.ascontiguousarray(comb, dtype=np.float64)
    n, n_script = len(work), int(n_script)
    if not (len(fan) == len(orig) == len(comb) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    words = np.zeros(n_script, dtype=abi.QUOTE_WORD_DTYPE)
    cap = min(n, (n_script + 1) // 2, 4096)         # regions lie a word apart at least
    while True:
        regions = np.empty(cap, dtype=abi.QUOTE_REGION_DTYPE)
        got = C.c_uint64(0)
        rc = L.fs_quotes(int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
                         abi.ptr(orig, C.c_uint32), abi.ptr(comb, C.c_double), n, int(n_works),
                         n_script, int(min_words), int(max_gap), int(min_works),
                         words.ctypes.data_as(C.c_void_p), regions.ctypes.data_as(C.c_void_p),
                         cap, C.byref(got))
        if rc == abi.FS_E_CAPACITY:
            cap = int(got.value)
            continue
        _lib.check(rc, "fs_quotes")
        return words, regions[:got.value]


def word_labels(rows):
    """{script word index: (word, character, scene)} of the records `rows`; ValueError for a
    script word that carries two different texts, characters or scenes."""
    labels = {}
    for r in rows:
        o = int(r[_ORIG_IX])
        lab = (r[_ORIG_WORD], r[_CHAR], r[_SCENE])
        have = labels.setdefault(o, lab)
        if have != lab:
            what, a, b = next((w, x, y) for w, x, y in zip(('word', 'character', 'scene'), have, lab)
                              if x != y)
            raise ValueError("script word %d has two %ss, %r and %r: records of different "
                             "scripts in one file?" % (o, what, a, b))
    return labels


def tables(rows, min_words=6, max_gap=0, min_works=1, device=0):
    """(regions, words): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    n_works = len(set(r[_FNAME] for r in rows))
    n_script = int(orig.max()) + 1 if len(orig) else 0
    return _tables(labels, work, fan, orig, comb, n_works, n_script, min_words, max_gap,
                   min_works, device)


def tables_device(mf, min_words=6, max_gap=0, min_works=1, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = int(orig.max()) + 1 if len(orig) else 0
    cols = [mf.labels(c, n_script) for c in (_ORIG_WORD, _CHAR, _SCENE)]
    if any(c is None for c in cols):
        return None
    labels = {o: (w, cols[1][o], cols[2][o]) for o, w in cols[0].items()}
    return _tables(labels, work, fan, orig, comb, len(mf.names), n_script, min_words, max_gap,
                   min_works, device)


def _tables(labels, work, fan, orig, comb, n_works, n_script, min_words, max_gap, min_works,
            device):
    words, regions = find_quotes(work, fan, orig, comb, n_works, n_script, min_words, max_gap,
                                 min_works, device)
    unknown = (UNKNOWN_WORD, '', '')
    rtab = []
    for r in regions:
        a, b = int(r['first']), int(r['last'])
        _, char, scene = labels[a]                  # a region starts at a record
        rtab.append([a, b, b - a + 1, char, scene, int(r['n_passages']), int(r['n_works']),
                     int(r['n_words']), int(r['n_exact']), int(r['peak']), int(r['peak_first']),
                     int(r['peak_last']),
                     ' '.join(labels.get(o, unknown)[0] for o in range(a, b + 1))])
    wtab = []
    for o in np.nonzero((words['n_words'] > 0) | (words['n_passages'] > 0))[0].tolist():
        w = words[o]
        region = int(w['region'])
        wtab.append([o, labels.get(o, unknown)[0], int(w['n_words']), int(w['n_exact']),
                     int(w['n_works']), int(w['n_passages']), int(w['n_passage_works']),
                     '' if region == abi.FS_NONE else region + 1])
    return rtab, wtab


def output_names(matches, prefix=None):
    if prefix is None:
        prefix = matches[:-4] if matches.endswith('.csv') else matches
    return (prefix + '-quotes.csv', prefix + '-quotes-words.csv')


def process(args):
    """`ao3.py quotes matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-works K]
    [--device D] [--reader {device,python}]`."""
    from .matches import MatchFile, reader_of
    outs = output_names(args.matches, args.output)
    body = None
    if reader_of(args) == 'device':
        with MatchFile(args.matches, args.device) as mf:
            if not mf.outside:
                body = tables_device(mf, args.min_words, args.max_gap, args.min_works,
                                     args.device)
    if body is None:        # the python reader, or a file the device reader does not take
        body = tables(read_matches(args.matches), args.min_words, args.max_gap, args.min_works,
                      args.device)
    for path, head, part in zip(outs, (REGION_FIELDS, WORD_FIELDS), body):
        with open(path, 'w', newline='', encoding='utf-8') as fh:
            w = csv.writer(fh)
            w.writerow(head)
            w.writerows(part)
    return outs
