"""`ao3.py companions`: the quoted stretches of a script related to each other by the fan works
that quote them.

`pairs` asks which works quote the same material; this command asks the transposed question:
do the works that quote this line also quote that one, which scenes travel together?  A unit is
a region of `quotes` (`--by region`), a scene or a character of the script.  A work quotes a
unit when a passage of it covers a script word of the unit (bridged words included); a pair of
units has in common the works quoting both, and the pairs with at least `--min-both` such works,
making up at least `--min-share` percent of the works of the less quoted unit, are listed with
the usual overlap figures, ranked by the number of common works; per unit, its works, the number
of its partners and the closest one.

Reading, sorting (passages.read_matches / sort_records), the unit map and writing are host
plumbing; the passages, the unit x work incidence matrix and the unit x unit product come from
the GPU (fs_companions), the regions from fs_quotes.  A passage is what `passages` keeps under
the same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi, quotes
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels
from .works import groups_of_labels

BY = ('region', 'scene', 'character')
PAIR_FIELDS = ['A', 'B', 'A_FIRST_WORD_INDEX', 'A_LAST_WORD_INDEX', 'A_CHARACTER', 'A_SCENE',
               'A_WORKS', 'B_FIRST_WORD_INDEX', 'B_LAST_WORD_INDEX', 'B_CHARACTER', 'B_SCENE',
               'B_WORKS', 'BOTH', 'EITHER', 'JACCARD_PERCENT', 'SHARE_PERCENT', 'LIFT_PERMILLE',
               'FIRST_FAN_WORK_FILENAME', 'A_TEXT', 'B_TEXT']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'PARTNERS', 'BEST_PARTNER', 'BEST_BOTH', 'TEXT']


def find_companions(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                    max_gap=0, min_both=2, min_share=0, device=0):
    """(abi.COMPANION_UNIT_DTYPE[n_units], abi.COMPANION_DTYPE pairs in (a, b) order) of records
    sorted by (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script words."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units = len(work), int(n_units)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    L = _lib.load()
    units = np.zeros(n_units, dtype=abi.COMPANION_UNIT_DTYPE)
    pairs = grow(lambda out, cap, got: L.fs_companions(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), int(min_both), int(min_share),
        units.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.COMPANION_DTYPE, 4096, "fs_companions")
    return units, pairs


def active_works(work, fan_ix, orig_ix, min_words=6, max_gap=0):
    """How many works of the records sorted by (work, fan_ix) have a passage (the N of
    LIFT_PERMILLE; the join rule of `passages` on whole columns)."""
    work, fan, orig = (np.asarray(c).astype(np.int64) for c in (work, fan_ix, orig_ix))
    if not len(work):
        return 0
    df, do = np.diff(fan), np.diff(orig)
    joined = (np.diff(work) == 0) & (df >= 1) & (df <= 1 + max_gap) & (do >= 1) & (do <= 1 + max_gap)
    heads = np.concatenate(([0], np.nonzero(~joined)[0] + 1, [len(work)]))
    kept = heads[:-1][np.diff(heads) >= min_words]
    return len(np.unique(work[kept]))


def tables(rows, by='region', min_words=6, max_gap=0, min_works=1, min_both=2, min_share=0,
           device=0):
    """(pairs, units): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, min_both, min_share, device)


def tables_device(mf, by='region', min_words=6, max_gap=0, min_works=1, min_both=2, min_share=0,
                  device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, min_both, min_share, device)


def units_of(labels, work, fan, orig, comb, n_works, n_script, by, min_words, max_gap, min_works,
             device):
    """(unit_of[n_script], about): the unit of every script word and, per unit, (first word,
    last word, character, scene, text)."""
    unknown = (UNKNOWN_WORD, '', '')
    if by == 'region':
        words, regions = quotes.find_quotes(work, fan, orig, comb, n_works, n_script, min_words,
                                            max_gap, min_works, device)
        about = []
        for r in regions:
            a, b = int(r['first']), int(r['last'])
            _, char, scene = labels[a]              # a region starts at a record
            about.append((a, b, char, scene,
                          ' '.join(labels.get(o, unknown)[0] for o in range(a, b + 1))))
        return abi.as_u32(words['region']), about
    col = {'character': 1, 'scene': 2}[by]
    group_of, found = groups_of_labels({o: lab[col] for o, lab in labels.items()}, n_script)
    unit_of = np.full(n_script, abi.FS_NONE, dtype=np.uint32)
    at = np.fromiter(labels, dtype=np.int64, count=len(labels))
    unit_of[at] = group_of[at]                      # a word without a record has no unit
    first, last = {}, {}
    for o in sorted(labels):
        u = int(group_of[o])
        first.setdefault(u, o)
        last[u] = o
    about = [(first[u], last[u], name if col == 1 else '', name if col == 2 else '', '')
             for u, name in enumerate(found)]
    return unit_of, about


def word_units_of(labels, work, fan, orig, comb, n_works, n_script, min_words, max_gap, min_works,
                  device):
    """(unit_of[n_script], about) of `intervals --by word`: every script word inside a region of
    `quotes` is a unit of its own, numbered in script order; its character, scene and text are
    the word's own, those of a bridged word no record names unknown."""
    words, _ = quotes.find_quotes(work, fan, orig, comb, n_works, n_script, min_words, max_gap,
                                  min_works, device)
    at = np.nonzero(abi.as_u32(words['region']) != abi.FS_NONE)[0]
    unit_of = np.full(n_script, abi.FS_NONE, dtype=np.uint32)
    unit_of[at] = np.arange(len(at), dtype=np.uint32)
    unknown = (UNKNOWN_WORD, '', '')
    about = []
    for o in at.tolist():
        word, char, scene = labels.get(o, unknown)
        about.append((o, o, char, scene, word))
    return unit_of, about


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            min_both, min_share, device):
    if by not in BY:
        raise ValueError("--by %r: region, scene or character" % (by,))
    unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by, min_words,
                              max_gap, min_works, device)
    units, pairs = find_companions(work, fan, orig, len(names), n_script, unit_of, len(about),
                                   min_words, max_gap, min_both, min_share, device)
    n_active = active_works(work, fan, orig, min_words, max_gap)
    # BOTH descending, then unit A, then unit B (the device's order, kept by a stable sort)
    order = np.argsort(-pairs['both'].astype(np.int64), kind='stable')
    ptab = []
    for p in pairs[order]:
        a, b, n = int(p['a']), int(p['b']), int(p['both'])
        wa, wb = int(p['works_a']), int(p['works_b'])
        either = wa + wb - n
        ptab.append([a + 1, b + 1] + list(about[a][:4]) + [wa] + list(about[b][:4]) + [wb]
                    + [n, either, n * 100 // either, n * 100 // min(wa, wb),
                       n * n_active * 1000 // (wa * wb), names[int(p['first_work'])],
                       about[a][4], about[b][4]])
    utab = []
    for u, v in enumerate(units):
        best = int(v['best'])
        utab.append([u + 1] + list(about[u][:4])
                    + [int(v['works']), int(v['partners']),
                       '' if best == abi.FS_NONE else best + 1, int(v['best_both']), about[u][4]])
    return ptab, utab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-companions.csv', '-companions-units.csv'))


def process(args):
    """`ao3.py companions matches [-o PREFIX] [--by region|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--min-both B] [--min-share P] [--device D]
    [--reader {device,python}]`."""
    opts = (args.by, args.min_words, args.max_gap, args.min_works, args.min_both, args.min_share,
            args.device)
    return run(args, (PAIR_FIELDS, UNIT_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
