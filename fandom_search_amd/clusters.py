"""`ao3.py clusters`: the families of fan works of a match CSV that quote the same lines.

`pairs` lists every two works sharing script words, which a large fandom makes unreadable:
thousands of works quoting the same twenty stretches are millions of pairs.  This command gives
the structure of that product.  Two works are linked when their coverages share at least
`--min-shared` words and that is at least `--min-jaccard` per cent of the words either covers;
a family is a connected component of the links (two works that share nothing may be in one
through a third); per family of at least `--min-size` works, its size, its links, the work in
its middle (the most links), the script words any member covers, those at least `--common` per
cent of the members cover and their longest run; per work, its family, its links and its
closest linked partner.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the coverage bitsets, the work x work product, the components and the per-family
reduction come from the GPU (fs_clusters), and no pair is ever listed.  A passage is what
`passages` keeps under the same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels

CLUSTER_FIELDS = ['CLUSTER', 'WORKS', 'LINKS', 'HUB_FAN_WORK_FILENAME', 'HUB_LINKS',
                  'COVERED_WORDS', 'COMMON_WORDS', 'PEAK_WORKS', 'PEAK_WORD_INDEX',
                  'COMMON_RUN_START', 'COMMON_RUN_WORDS', 'COMMON_RUN_CHARACTER',
                  'COMMON_RUN_SCENE', 'COMMON_RUN_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'CLUSTER', 'CLUSTER_WORKS', 'COVERED_WORDS', 'LINKS',
               'BEST_PARTNER', 'BEST_SHARED_WORDS']


def find_clusters(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0,
                  min_shared=6, min_jaccard=50, min_size=2, common_pct=50, device=0):
    """(abi.CLUSTER_WORK_DTYPE[n_works], abi.CLUSTER_DTYPE listed families in ascending order
    of root) of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n, n_works = len(work), int(n_works)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.CLUSTER_WORK_DTYPE)
    found = grow(lambda out, cap, got: L.fs_clusters(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, n_works, int(n_script), int(min_words), int(max_gap),
        int(min_shared), int(min_jaccard), int(min_size), int(common_pct),
        works.ctypes.data_as(C.c_void_p), out, cap, got), abi.CLUSTER_DTYPE, 4096, "fs_clusters")
    return works, found


def tables(rows, min_words=6, max_gap=0, min_shared=6, min_jaccard=50, min_size=2,
           common_pct=50, device=0):
    """(clusters, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), min_words,
                   max_gap, min_shared, min_jaccard, min_size, common_pct, device)


def tables_device(mf, min_words=6, max_gap=0, min_shared=6, min_jaccard=50, min_size=2,
                  common_pct=50, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, n_script, min_words, max_gap,
                   min_shared, min_jaccard, min_size, common_pct, device)


def _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, min_shared,
            min_jaccard, min_size, common_pct, device):
    works, found = find_clusters(work, fan, orig, len(names), n_script, min_words, max_gap,
                                 min_shared, min_jaccard, min_size, common_pct, device)
    unknown = (UNKNOWN_WORD, '', '')
    # WORKS descending, then the root (the device's order, kept by a stable sort)
    order = np.argsort(-found['n_works'].astype(np.int64), kind='stable')
    rank = np.empty(len(found), dtype=np.int64)
    rank[order] = np.arange(1, len(found) + 1)
    ctab = []
    for k in order.tolist():
        c = found[k]
        s, n = int(c['run_first']), int(c['run_words'])
        if int(c['common']):
            _, char, scene = labels.get(s, unknown)
            run = [s, n, char, scene,
                   ' '.join(labels.get(o, unknown)[0] for o in range(s, s + n))]
        else:               # no word is common: no start, character, scene or text
            run = ['', 0, '', '', '']
        ctab.append([int(rank[k]), int(c['n_works']), int(c['n_links']), names[int(c['hub'])],
                     int(c['hub_links']), int(c['covered']), int(c['common']), int(c['peak']),
                     int(c['peak_first'])] + run)
    wtab = []
    for w in np.nonzero(works['covered'])[0].tolist():
        v = works[w]
        best, cluster = int(v['best']), int(v['cluster'])
        wtab.append([names[w], '' if cluster == abi.FS_NONE else int(rank[cluster]),
                     int(v['size']), int(v['covered']), int(v['links']),
                     '' if best == abi.FS_NONE else names[best], int(v['best_shared'])])
    return ctab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-clusters.csv', '-clusters-works.csv'))


def process(args):
    """`ao3.py clusters matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-shared S]
    [--min-jaccard J] [--min-size N] [--common P] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.min_shared, args.min_jaccard, args.min_size,
            args.common, args.device)
    return run(args, (CLUSTER_FIELDS, WORK_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
