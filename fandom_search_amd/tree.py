"""`ao3.py tree`: how the families of the fan works of a match CSV merge as the bar drops.

`clusters` gives the families at one bar, `--min-jaccard`, that has to be guessed in advance.
This command gives every bar at once, the single-linkage dendrogram: two works have an edge when
their coverages share at least `--min-shared` words, the edge's level is the Jaccard of the two
coverages in parts per million (`--measure jaccard`) or the shared words themselves (`--measure
shared`), the edges are taken from the highest level down (then the earlier work A, then the
earlier work B), and an edge whose works are in different families merges the two.  Per merge
its level, its edge with what the two works share, the two sides and the merged family; per work
its tree, its first merge and its place in a leaf order that puts relatives next to each other;
per level the families there are once every merge at that level or above is made, which is how
to choose a bar for `clusters`.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the coverage bitsets, the work x work product and the forest come from the GPU, the
replay of its at most N - 1 edges from the library's host code (fs_tree), and no pair is ever
listed.  A passage is what `passages` keeps under the same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels

MERGE_FIELDS = ['MERGE', 'LEVEL', 'A_FAN_WORK_FILENAME', 'B_FAN_WORK_FILENAME', 'SHARED_WORDS',
                'A_COVERED_WORDS', 'B_COVERED_WORDS', 'LEFT', 'RIGHT', 'LEFT_WORKS',
                'RIGHT_WORKS', 'WORKS', 'FIRST_FAN_WORK_FILENAME', 'TREE', 'SHARED_RUN_START',
                'SHARED_RUN_WORDS', 'SHARED_RUN_CHARACTER', 'SHARED_RUN_SCENE',
                'SHARED_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'TREE', 'TREE_WORKS', 'EDGES',
               'JOINED_AT_MERGE', 'JOINED_AT_LEVEL', 'BEST_PARTNER', 'LEAF_ORDER']
LEVEL_FIELDS = ['LEVEL', 'MERGES', 'FAMILIES', 'LARGEST_WORKS', 'SINGLE_WORKS']


def measure_code(measure):
    if measure not in abi.TREE_MEASURES:
        raise ValueError("measure must be jaccard or shared")
    return abi.TREE_MEASURES.index(measure)


def find_tree(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0,
              measure='jaccard', min_shared=6, min_level=0, device=0):
    """(abi.TREE_WORK_DTYPE[n_works], abi.TREE_MERGE_DTYPE merges in merge order,
    abi.TREE_LEVEL_DTYPE levels, the highest first) of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n, n_works, code = len(work), int(n_works), measure_code(measure)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.TREE_WORK_DTYPE)
    merges, levels = grow(lambda m, cap_m, got_m, v, cap_v, got_v: L.fs_tree(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, n_works, int(n_script), int(min_words), int(max_gap), code,
        int(min_shared), int(min_level), works.ctypes.data_as(C.c_void_p), m, cap_m, got_m,
        v, cap_v, got_v), [abi.TREE_MERGE_DTYPE, abi.TREE_LEVEL_DTYPE], [4096, 256], "fs_tree")
    return works, merges, levels


def tables(rows, min_words=6, max_gap=0, measure='jaccard', min_shared=6, min_level=0,
           device=0):
    """(merges, works, levels): the three CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), min_words,
                   max_gap, measure, min_shared, min_level, device)


def tables_device(mf, min_words=6, max_gap=0, measure='jaccard', min_shared=6, min_level=0,
                  device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, n_script, min_words, max_gap,
                   measure, min_shared, min_level, device)


def _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, measure, min_shared,
            min_level, device):
    works, merges, levels = find_tree(work, fan, orig, len(names), n_script, min_words, max_gap,
                                      measure, min_shared, min_level, device)
    unknown = (UNKNOWN_WORD, '', '')

    def side(k):
        return '' if k == abi.FS_NONE else k + 1

    mtab = []
    for k, m in enumerate(merges.tolist()):
        (a, b, level, shared, ca, cb, left, right, n_left, n_right, n, first, tree, s, run,
         _) = m
        _, char, scene = labels.get(s, unknown)
        mtab.append([k + 1, level, names[a], names[b], shared, ca, cb, side(left), side(right),
                     n_left, n_right, n, names[first], tree + 1, s, run, char, scene,
                     ' '.join(labels.get(o, unknown)[0] for o in range(s, s + run))])
    wtab = []
    for w in np.nonzero(works['covered'])[0].tolist():
        covered, tree, n, edges, merge, level, best, leaf = works[w].tolist()
        joined = ['', '', ''] if merge == abi.FS_NONE else [merge + 1, level, names[best]]
        wtab.append([names[w], covered, tree + 1, n, edges] + joined + [leaf])
    ltab = [[v['level'], v['merges'], v['families'], v['largest'], v['singles']]
            for v in ({n: int(x[n]) for n in x.dtype.names} for x in levels)]
    return mtab, wtab, ltab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-tree.csv', '-tree-works.csv', '-tree-levels.csv'))


def process(args):
    """`ao3.py tree matches [-o PREFIX] [--measure {jaccard,shared}] [--min-shared S]
    [--min-level L] [--min-words M] [--max-gap G] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.measure, args.min_shared, args.min_level,
            args.device)
    return run(args, (MERGE_FIELDS, WORK_FIELDS, LEVEL_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
