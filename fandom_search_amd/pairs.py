"""`ao3.py pairs`: the fan works of a match CSV related to each other by what they take from
the script.

`quotes` says which stretches of the script are quoted and by how many works.  This command
answers which works quote the same material: the coverage of a work is every script word its
passages cover (bridged ones included), a pair of works shares the words in both coverages, and
the pairs sharing at least `--min-shared` words are listed with where the shared words lie and
their longest run, ranked by the number of shared words; per work, its coverage, the number of
its partners and the closest one.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the coverage bitsets and the work x work product come from the GPU (fs_pairs).  A
passage is what `passages` keeps under the same `--min-words` and `--max-gap`.
"""

import csv
import ctypes as C

import numpy as np

from . import _lib, abi
from .passages import _CHAR, _FNAME, _ORIG_WORD, _SCENE, read_matches, sort_records
from .quotes import UNKNOWN_WORD, word_labels

PAIR_FIELDS = ['FAN_WORK_FILENAME_A', 'FAN_WORK_FILENAME_B', 'COVERED_WORDS_A',
               'COVERED_WORDS_B', 'SHARED_WORDS', 'FIRST_SHARED_WORD_INDEX',
               'LAST_SHARED_WORD_INDEX', 'LONGEST_RUN_START', 'LONGEST_RUN_WORDS',
               'LONGEST_RUN_CHARACTER', 'LONGEST_RUN_SCENE', 'LONGEST_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'PARTNERS', 'BEST_PARTNER',
               'BEST_SHARED_WORDS']


def find_pairs(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0, min_shared=6,
               device=0):
    """(abi.PAIR_WORK_DTYPE[n_works], abi.PAIR_DTYPE pairs in (a, b) order) of records sorted
    by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n, n_works = len(work), int(n_works)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.PAIR_WORK_DTYPE)
    cap = 4096
    while True:
        pairs = np.empty(cap, dtype=abi.PAIR_DTYPE)
        got = C.c_uint64(0)
        rc = L.fs_pairs(int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
                        abi.ptr(orig, C.c_uint32), n, n_works, int(n_script), int(min_words),
                        int(max_gap), int(min_shared), works.ctypes.data_as(C.c_void_p),
                        pairs.ctypes.data_as(C.c_void_p), cap, C.byref(got))
        if rc == abi.FS_E_CAPACITY:
            cap = int(got.value)
            continue
        _lib.check(rc, "fs_pairs")
        return works, pairs[:got.value]


def tables(rows, min_words=6, max_gap=0, min_shared=6, device=0):
    """(pairs, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    names = list(dict.fromkeys(r[_FNAME] for r in rows))
    n_script = int(orig.max()) + 1 if len(orig) else 0
    return _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, min_shared,
                   device)


def tables_device(mf, min_words=6, max_gap=0, min_shared=6, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = int(orig.max()) + 1 if len(orig) else 0
    cols = [mf.labels(c, n_script) for c in (_ORIG_WORD, _CHAR, _SCENE)]
    if any(c is None for c in cols):
        return None
    labels = {o: (w, cols[1][o], cols[2][o]) for o, w in cols[0].items()}
    return _tables(labels, list(mf.names), work, fan, orig, n_script, min_words, max_gap,
                   min_shared, device)


def _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, min_shared, device):
    works, pairs = find_pairs(work, fan, orig, len(names), n_script, min_words, max_gap,
                              min_shared, device)
    unknown = (UNKNOWN_WORD, '', '')
    covered = works['covered']
    # SHARED_WORDS descending, then work A, then work B (the device's order, kept by a stable sort)
    order = np.argsort(-pairs['shared'].astype(np.int64), kind='stable')
    ptab = []
    for p in pairs[order]:
        a, b, s, n = int(p['a']), int(p['b']), int(p['run_first']), int(p['run_words'])
        _, char, scene = labels.get(s, unknown)
        ptab.append([names[a], names[b], int(covered[a]), int(covered[b]), int(p['shared']),
                     int(p['first']), int(p['last']), s, n, char, scene,
                     ' '.join(labels.get(o, unknown)[0] for o in range(s, s + n))])
    wtab = []
    for w in np.nonzero(covered)[0].tolist():
        v = works[w]
        best = int(v['best'])
        wtab.append([names[w], int(v['covered']), int(v['partners']),
                     '' if best == abi.FS_NONE else names[best], int(v['best_shared'])])
    return ptab, wtab


def output_names(matches, prefix=None):
    if prefix is None:
        prefix = matches[:-4] if matches.endswith('.csv') else matches
    return (prefix + '-pairs.csv', prefix + '-pairs-works.csv')


def process(args):
    """`ao3.py pairs matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-shared S]
    [--device D] [--reader {device,python}]`."""
    from .matches import MatchFile, reader_of
    outs = output_names(args.matches, args.output)
    body = None
    if reader_of(args) == 'device':
        with MatchFile(args.matches, args.device) as mf:
            if not mf.outside:
                body = tables_device(mf, args.min_words, args.max_gap, args.min_shared,
                                     args.device)
    if body is None:        # the python reader, or a file the device reader does not take
        body = tables(read_matches(args.matches), args.min_words, args.max_gap, args.min_shared,
                      args.device)
    for path, head, part in zip(outs, (PAIR_FIELDS, WORK_FIELDS), body):
        with open(path, 'w', newline='', encoding='utf-8') as fh:
            w = csv.writer(fh)
            w.writerow(head)
            w.writerows(part)
    return outs
