"""`ao3.py routes`: the sequences of quoted stretches of a script that the fan works quote in
that order.

`transitions` relates the units one step at a time; a fandom that retells three scenes in a
row is two unrelated cells there, and a work that quotes something else in between breaks the
chain.  This command lists the routes themselves, the ordered counterpart of `bundles`: every
sequence of 2 to `--max-length` units (the units of `companions`: regions of `quotes`, scenes
or characters) that at least `--min-all` works quote in that order, with at most `--max-skip`
other elements of a work's sequence between two units of the route (default: any distance).
A work's sequence is its unit-bearing passages in record order, consecutive passages of one
unit written once, as `retellings` collapses SCENE_SEQUENCE.  Per route the works, the works of
the route without its last unit and the share of them that go on, the direction in the script,
whether the route is closed (no frequent route with a unit more in front or behind has the
same works) and how many frequent routes continue it either way.  Closed routes only, unless
`--all`.  Per unit the routes holding it; per length the candidates and the frequent and
closed routes, which is how to choose `--min-all` and `--max-length`.

Reading, sorting, the unit map (companions.units_of) and writing are host plumbing; the
passages, the sequences, their bitmaps and the level-wise mining come from the GPU (fs_routes).
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .companions import BY, units_of
from .passages import sort_records
from .quotes import word_labels

ROUTE_FIELDS = ['ROUTE', 'LENGTH', 'UNITS', 'WORKS', 'PREFIX_WORKS', 'CONTINUE_PERCENT',
                'DIRECTION', 'CLOSED', 'FORWARD', 'BACKWARD', 'FIRST_FAN_WORK_FILENAME',
                'FIRST_WORD_INDEXES', 'CHARACTERS', 'SCENES', 'TEXTS']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'ROUTES', 'LONGEST_ROUTE', 'BEST_ROUTE', 'TEXT']
LEVEL_FIELDS = ['LENGTH', 'CANDIDATES', 'FREQUENT', 'CLOSED', 'PRINTED']
JOIN = ' | '
THEN = ' > '


def find_routes(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                max_gap=0, max_skip=None, min_all=5, max_length=4, device=0):
    """(abi.ROUTE_UNIT_DTYPE[n_units], abi.ROUTE_LEVEL_DTYPE[max_length] for the lengths 2 ..
    max_length + 1, abi.ROUTE_DTYPE routes by length, then lexicographically) of records sorted
    by (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script words.  max_skip
    None (or abi.FS_NONE): any distance."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units = len(work), int(n_units)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    skip = abi.FS_NONE if max_skip is None else int(max_skip)
    L = _lib.load()
    units = np.zeros(n_units, dtype=abi.ROUTE_UNIT_DTYPE)
    levels = np.zeros(max(1, int(max_length)), dtype=abi.ROUTE_LEVEL_DTYPE)
    routes = grow(lambda out, cap, got: L.fs_routes(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), skip, int(min_all), int(max_length),
        units.ctypes.data_as(C.c_void_p), levels.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.ROUTE_DTYPE, 4096, "fs_routes")
    return units, levels, routes


def direction(units):
    """`forward` when the unit numbers strictly ascend, `back` when they strictly descend."""
    if all(b > a for a, b in zip(units, units[1:])):
        return 'forward'
    if all(b < a for a, b in zip(units, units[1:])):
        return 'back'
    return 'mixed'


def tables(rows, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_length=4,
           max_skip=None, every=False, device=0):
    """(routes, units, levels): the three CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, min_all, max_length, max_skip, every, device)


def tables_device(mf, by='region', min_words=6, max_gap=0, min_works=1, min_all=5, max_length=4,
                  max_skip=None, every=False, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, min_all, max_length, max_skip, every, device)


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            min_all, max_length, max_skip, every, device):
    if by not in BY:
        raise ValueError("--by %r: region, scene or character" % (by,))
    if min_all < 1:
        raise ValueError("--min-all must be at least 1")
    if not 2 <= max_length <= abi.FS_ROUTES_MAX_LENGTH:
        raise ValueError("--max-length must be from 2 to %d" % abi.FS_ROUTES_MAX_LENGTH)
    if max_skip is not None and not 0 <= max_skip <= abi.FS_ROUTES_MAX_SKIP:
        raise ValueError("--max-skip must be from 0 to %d" % abi.FS_ROUTES_MAX_SKIP)
    unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by, min_words,
                              max_gap, min_works, device)
    try:
        units, levels, routes = find_routes(work, fan, orig, len(names), n_script, unit_of,
                                            len(about), min_words, max_gap, max_skip, min_all,
                                            max_length, device)
    except _lib.FsError as e:
        if e.code != abi.FS_E_UNSUPPORTED:
            raise
        raise ValueError(str(e))                    # the cap on a level, the tables' bytes
    listed = []
    for r in routes:
        k = int(r['length'])
        if every or int(r['closed']):
            listed.append((-int(r['works']), -k, tuple(int(u) for u in r['units'][:k]), r))
    listed.sort(key=lambda t: t[:3])
    rtab, best, printed = [], {}, {}
    for row, (_, _, us, r) in enumerate(listed, 1):
        n, before = int(r['works']), int(r['prefix_works'])
        for u in us:
            best.setdefault(u, row)
        printed[len(us)] = printed.get(len(us), 0) + 1
        rtab.append([row, len(us), THEN.join(str(u + 1) for u in us), n, before,
                     n * 100 // before, direction(us), int(r['closed']), int(r['forward']),
                     int(r['backward']), names[int(r['first_work'])],
                     ' '.join(str(about[u][0]) for u in us),
                     JOIN.join(about[u][2] for u in us), JOIN.join(about[u][3] for u in us),
                     JOIN.join(about[u][4] for u in us) if by == 'region' else ''])
    utab = []
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [int(v['works']), int(v['routes']), int(v['longest']), best.get(u, ''),
                       about[u][4]])
    ltab = []
    for v in levels:
        k = int(v['length'])
        ltab.append([k, int(v['candidates']), int(v['frequent']),
                     '' if k > max_length else int(v['closed']), printed.get(k, 0)])
    return rtab, utab, ltab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-routes.csv', '-routes-units.csv', '-routes-levels.csv'))


def process(args):
    """`ao3.py routes matches [-o PREFIX] [--by region|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--min-all A] [--max-length L] [--max-skip S] [--all]
    [--device D] [--reader {device,python}]`."""
    opts = (args.by, args.min_words, args.max_gap, args.min_works, args.min_all,
            args.max_length, args.max_skip, args.all, args.device)
    return run(args, (ROUTE_FIELDS, UNIT_FIELDS, LEVEL_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
