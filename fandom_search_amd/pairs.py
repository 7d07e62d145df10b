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

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
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
    pairs = grow(lambda out, cap, got: L.fs_pairs(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, n_works, int(n_script), int(min_words), int(max_gap),
        int(min_shared), works.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.PAIR_DTYPE, 4096, "fs_pairs")
    return works, pairs


def tables(rows, min_words=6, max_gap=0, min_shared=6, device=0):
    """(pairs, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), min_words,
                   max_gap, min_shared, device)


def tables_device(mf, min_words=6, max_gap=0, min_shared=6, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
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
    return prefixed(matches, prefix, ('-pairs.csv', '-pairs-works.csv'))


def process(args):
    """`ao3.py pairs matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-shared S]
    [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.min_shared, args.device)
    return run(args, (PAIR_FIELDS, WORK_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
