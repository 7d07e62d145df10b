"""`ao3.py neighbours`: each fan work's closest works by the rare lines both quote.

`pairs` and `clusters` relate the works by the script words both quote, every word counting the
same: a line half the fandom quotes links everything to everything, and no work has a ranking
of its own.  Here a script word weighs the more the fewer works cover it (`--weight rarity`:
the bits of active works // depth, 1 for a word more than half the works cover; `--weight
flat`: 1), the score of two works is the weight of the words in both coverages, their
similarity the weighted Jaccard in parts per million, and every work gets the list of its
`--top` closest works: with what they share, the rarest shared word and the run of shared words
around it, and whether the neighbour lists the work back.  A second file says per work how
obscure its quoting is and how the lists hold it, a third gives every covered script word's depth
and weight.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the coverage bitsets, the weights, the work x work product with its selection and the
details of the listed pairs come from the GPU (fs_neighbours).  A passage is what `passages`
keeps under the same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels

WEIGHT = ('rarity', 'flat')
NEIGHBOUR_FIELDS = ['FAN_WORK_FILENAME', 'RANK', 'NEIGHBOUR_FILENAME', 'SIMILARITY_PPM', 'SCORE',
                    'OWN_SCORE', 'NEIGHBOUR_OWN_SCORE', 'SHARED_WORDS', 'COVERED_WORDS',
                    'NEIGHBOUR_COVERED_WORDS', 'MUTUAL', 'BACK_RANK', 'RAREST_WORD_INDEX',
                    'RAREST_WORD', 'RAREST_DEPTH', 'RAREST_WEIGHT', 'RUN_FIRST_WORD_INDEX',
                    'RUN_WORDS', 'CHARACTER', 'SCENE', 'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'OWN_SCORE', 'RARITY_MILLI', 'CANDIDATES',
               'LISTED', 'LISTED_BY', 'MUTUAL', 'NEAREST', 'NEAREST_PPM']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'CHARACTER', 'SCENE',
               'DEPTH', 'WEIGHT']


def weight_code(weight):
    if weight not in WEIGHT:
        raise ValueError("--weight %r: rarity or flat" % (weight,))
    return abi.FS_NEIGHBOURS_FLAT if weight == 'flat' else abi.FS_NEIGHBOURS_RARITY


def find_neighbours(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0,
                    weight='rarity', top=10, min_score=1, min_similarity=0, device=0):
    """(abi.NEIGHBOUR_WORK_DTYPE[n_works], abi.NEIGHBOUR_WORD_DTYPE[n_script],
    abi.NEIGHBOUR_DTYPE listed pairs in (work, rank) order) of records sorted by
    (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n, n_works, n_script = len(work), int(n_works), int(n_script)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    code = weight_code(weight)
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.NEIGHBOUR_WORK_DTYPE)
    words = np.zeros(n_script, dtype=abi.NEIGHBOUR_WORD_DTYPE)
    listed = grow(lambda out, cap, got: L.fs_neighbours(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, n_works, n_script, int(min_words), int(max_gap), code,
        int(top), int(min_score), int(min_similarity), works.ctypes.data_as(C.c_void_p),
        words.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.NEIGHBOUR_DTYPE, 4096, "fs_neighbours")
    return works, words, listed


def tables(rows, weight='rarity', top=10, min_score=1, min_similarity=0, min_words=6, max_gap=0,
           device=0):
    """(neighbours, works, words): the three CSVs' rows, without headers, for the records
    `rows` (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), weight, top,
                   min_score, min_similarity, min_words, max_gap, device)


def tables_device(mf, weight='rarity', top=10, min_score=1, min_similarity=0, min_words=6,
                  max_gap=0, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, n_script, weight, top, min_score,
                   min_similarity, min_words, max_gap, device)


def _tables(labels, names, work, fan, orig, n_script, weight, top, min_score, min_similarity,
            min_words, max_gap, device):
    works, words, listed = find_neighbours(work, fan, orig, len(names), n_script, min_words,
                                           max_gap, weight, top, min_score, min_similarity,
                                           device)
    unknown = (UNKNOWN_WORD, '', '')
    covered, own = works['covered'], works['own']
    ntab = []
    for p in listed:                                     # (work, rank) order: the device's
        a, b, back = int(p['a']), int(p['b']), int(p['back_rank'])
        rare, s, n = int(p['rarest']), int(p['run_first']), int(p['run_words'])
        _, char, scene = labels.get(s, unknown)
        ntab.append([names[a], int(p['rank']), names[b], int(p['ppm']), int(p['score']),
                     int(own[a]), int(own[b]), int(p['shared']), int(covered[a]),
                     int(covered[b]), int(back != abi.FS_NONE),
                     '' if back == abi.FS_NONE else back, rare, labels.get(rare, unknown)[0],
                     int(p['rarest_depth']), int(p['rarest_weight']), s, n, char, scene,
                     ' '.join(labels.get(o, unknown)[0] for o in range(s, s + n))])
    wtab = []
    for w in np.nonzero(covered)[0].tolist():
        v = works[w]
        near = int(v['nearest'])
        wtab.append([names[w], int(v['covered']), int(v['own']),
                     int(v['own']) * 1000 // int(v['covered']), int(v['candidates']),
                     int(v['listed']), int(v['listed_by']), int(v['mutual']),
                     '' if near == abi.FS_NONE else names[near], int(v['nearest_ppm'])])
    otab = []
    for o in np.nonzero(words['depth'])[0].tolist():
        word, char, scene = labels.get(o, unknown)
        otab.append([o, word, char, scene, int(words[o]['depth']), int(words[o]['weight'])])
    return ntab, wtab, otab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-neighbours.csv', '-neighbours-works.csv', '-neighbours-words.csv'))


def process(args):
    """`ao3.py neighbours matches [-o PREFIX] [--weight rarity|flat] [--top K] [--min-score S]
    [--min-similarity P] [--min-words M] [--max-gap G] [--device D]
    [--reader {device,python}]`."""
    weight_code(args.weight)
    opts = (args.weight, args.top, args.min_score, args.min_similarity, args.min_words,
            args.max_gap, args.device)
    return run(args, (NEIGHBOUR_FIELDS, WORK_FIELDS, WORD_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
