"""`ao3.py bundles`: the sets of quoted stretches of a script that the same fan works quote.

`companions` relates the units two at a time; three lines that the same forty works all quote
are three unrelated rows there.  This command lists the sets themselves: every set of 2 to
`--max-size` units (the units of `companions`: regions of `quotes`, scenes or characters) that
at least `--min-all` works quote in full, with the works, the share of the least quoted unit's
works, the lift over independent quoting, whether the set is closed (no further unit is quoted
by all of its works) and how many frequent sets extend it.  Closed sets only, unless `--all`.
Per unit the sets holding it; per size the candidates, the frequent, closed and maximal sets,
which is how to choose `--min-all` and `--max-size`.

Reading, sorting, the unit map (companions.units_of) and writing are host plumbing; the
passages, the unit x work incidence matrix and the level-wise mining come from the GPU
(fs_bundles).  LIFT_PERMILLE is computed here, in Python integers: N ** 7 at a million works
fits no machine word.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .companions import BY, active_works, units_of
from .passages import sort_records
from .quotes import word_labels

SET_FIELDS = ['SET', 'SIZE', 'UNITS', 'WORKS', 'LEAST_UNIT_WORKS', 'SHARE_PERCENT',
              'LIFT_PERMILLE', 'CLOSED', 'EXTENSIONS', 'FIRST_FAN_WORK_FILENAME',
              'FIRST_WORD_INDEXES', 'CHARACTERS', 'SCENES', 'TEXTS']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'SETS', 'LARGEST_SET', 'BEST_SET', 'TEXT']
LEVEL_FIELDS = ['SIZE', 'CANDIDATES', 'FREQUENT', 'CLOSED', 'MAXIMAL', 'PRINTED']
JOIN = ' | '


def find_bundles(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                 max_gap=0, min_all=5, max_size=4, device=0):
    """(abi.BUNDLE_UNIT_DTYPE[n_units], abi.BUNDLE_LEVEL_DTYPE[max_size] for the sizes 2 ..
    max_size + 1, abi.BUNDLE_DTYPE sets by size, then lexicographically) of records sorted by
    (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script words."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units = len(work), int(n_units)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    L = _lib.load()
    units = np.zeros(n_units, dtype=abi.BUNDLE_UNIT_DTYPE)
    levels = np.zeros(max(1, int(max_size)), dtype=abi.BUNDLE_LEVEL_DTYPE)
    sets = grow(lambda out, cap, got: L.fs_bundles(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), int(min_all), int(max_size),
        units.ctypes.data_as(C.c_void_p), levels.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.BUNDLE_DTYPE, 4096, "fs_bundles")
    return units, levels, sets


def lift_permille(works, n_active, unit_works):
    """WORKS * N ** (SIZE - 1) * 1000 // the product of the units' works, in Python integers
    whatever the arguments are: 1000 is what independent quoting gives."""
    den = 1
    for w in unit_works:
        den *= int(w)
    return int(works) * int(n_active) ** (len(unit_works) - 1) * 1000 // den


def tables(rows, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_size=4,
           every=False, device=0):
    """(sets, units, levels): the three CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, min_all, max_size, every, device)


def tables_device(mf, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_size=4,
                  every=False, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, min_all, max_size, every, device)


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            min_all, max_size, every, device):
    if by not in BY:
        raise ValueError("--by %r: region, scene or character" % (by,))
    if min_all < 1:
        raise ValueError("--min-all must be at least 1")
    if not 2 <= max_size <= abi.FS_BUNDLES_MAX_SIZE:
        raise ValueError("--max-size must be from 2 to %d" % abi.FS_BUNDLES_MAX_SIZE)
    unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by, min_words,
                              max_gap, min_works, device)
    try:
        units, levels, sets = find_bundles(work, fan, orig, len(names), n_script, unit_of,
                                           len(about), min_words, max_gap, min_all, max_size,
                                           device)
    except _lib.FsError as e:
        if e.code != abi.FS_E_UNSUPPORTED:
            raise
        raise ValueError(str(e))                    # the cap on a level, the tables' bytes
    n_active = active_works(work, fan, orig, min_words, max_gap)
    uworks = [int(w) for w in units['works']]
    listed = []
    for s in sets:
        k = int(s['size'])
        if every or int(s['closed']):
            listed.append((-int(s['works']), -k, tuple(int(u) for u in s['units'][:k]), s))
    listed.sort(key=lambda t: t[:3])
    stab, best, printed = [], {}, {}
    for row, (_, _, us, s) in enumerate(listed, 1):
        n, ws = int(s['works']), [uworks[u] for u in us]
        for u in us:
            best.setdefault(u, row)
        printed[len(us)] = printed.get(len(us), 0) + 1
        stab.append([row, len(us), ' '.join(str(u + 1) for u in us), n, min(ws),
                     n * 100 // min(ws), lift_permille(n, n_active, ws), int(s['closed']),
                     int(s['extensions']), names[int(s['first_work'])],
                     ' '.join(str(about[u][0]) for u in us),
                     JOIN.join(about[u][2] for u in us), JOIN.join(about[u][3] for u in us),
                     JOIN.join(about[u][4] for u in us) if by == 'region' else ''])
    utab = []
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [int(v['works']), int(v['sets']), int(v['largest']), best.get(u, ''),
                       about[u][4]])
    ltab = []
    for v in levels:
        k, last = int(v['size']), int(v['size']) > max_size
        ltab.append([k, int(v['candidates']), int(v['frequent']),
                     '' if last else int(v['closed']), '' if last else int(v['maximal']),
                     printed.get(k, 0)])
    return stab, utab, ltab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-bundles.csv', '-bundles-units.csv',
                                      '-bundles-levels.csv'))


def process(args):
    """`ao3.py bundles matches [-o PREFIX] [--by region|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--min-all A] [--max-size S] [--all] [--device D]
    [--reader {device,python}]`."""
    opts = (args.by, args.min_words, args.max_gap, args.min_works, args.min_all, args.max_size,
            args.all, args.device)
    return run(args, (SET_FIELDS, UNIT_FIELDS, LEVEL_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
