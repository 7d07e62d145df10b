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

import csv
import ctypes as C

import numpy as np

from . import _lib, abi
from .passages import _CHAR, _FNAME, _ORIG_WORD, _SCENE, read_matches, sort_records
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
    cap = 4096
    while True:
        found = np.empty(cap, dtype=abi.CLUSTER_DTYPE)
        got = C.c_uint64(0)
        rc = L.fs_clusters(int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
                           abi.ptr(orig, C.c_uint32), n, n_works, int(n_script), int(min_words),
                           int(max_gap), int(min_shared), int(min_jaccard), int(min_size),
                           int(common_pct), works.ctypes.data_as(C.c_void_p),
                           found.ctypes.data_as(C.c_void_p), cap, C.byref(got))
        if rc == abi.FS_E_CAPACITY:
            cap = int(got.value)
            continue
        _lib.check(rc, "fs_clusters")
        return works, found[:got.value]


def tables(rows, min_words=6, max_gap=0, min_shared=6, min_jaccard=50, min_size=2,
           common_pct=50, device=0):
    """(clusters, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    names = list(dict.fromkeys(r[_FNAME] for r in rows))
    n_script = int(orig.max()) + 1 if len(orig) else 0
    return _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, min_shared,
                   min_jaccard, min_size, common_pct, device)


def tables_device(mf, min_words=6, max_gap=0, min_shared=6, min_jaccard=50, min_size=2,
                  common_pct=50, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = int(orig.max()) + 1 if len(orig) else 0
    cols = [mf.labels(c, n_script) for c in (_ORIG_WORD, _CHAR, _SCENE)]
    if any(c is None for c in cols):
        return None
    labels = {o: (w, cols[1][o], cols[2][o]) for o, w in cols[0].items()}
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
    if prefix is None:
        prefix = matches[:-4] if matches.endswith('.csv') else matches
    return (prefix + '-clusters.csv', prefix + '-clusters-works.csv')


def process(args):
    """`ao3.py clusters matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-shared S]
    [--min-jaccard J] [--min-size N] [--common P] [--device D] [--reader {device,python}]`."""
    from .matches import MatchFile, reader_of
    outs = output_names(args.matches, args.output)
    params = (args.min_words, args.max_gap, args.min_shared, args.min_jaccard, args.min_size,
              args.common, args.device)
    body = None
    if reader_of(args) == 'device':
        with MatchFile(args.matches, args.device) as mf:
            if not mf.outside:
                body = tables_device(mf, *params)
    if body is None:        # the python reader, or a file the device reader does not take
        body = tables(read_matches(args.matches), *params)
    for path, head, part in zip(outs, (CLUSTER_FIELDS, WORK_FIELDS), body):
        with open(path, 'w', newline='', encoding='utf-8') as fh:
            w = csv.writer(fh)
            w.writerow(head)
            w.writerows(part)
    return outs
