"""`ao3.py trends`: which stretches of the script the later fan works quote more, and which the
earlier ones.

`groups --by year` prints a column of counts per year with nothing to judge them by, and
`contrast` wants the years cut into two heaps first.  This command keeps the order: every work
of the match file with a publication date has a period (`--by year` or `month`), and for every
unit (a region of `quotes`, a script word inside one, a scene or a character) it prints whether
the works quoting it are later or earlier than the works as a whole, by how much, how often a
random re-dating of the same works shifts them at least as far, and how often the largest
standardised shift over all units of a re-dating is as large: the max-statistic correction of
`contrast`.  A re-dating gives every dated work the date of a dated work drawn at random, with
replacement.  A second file counts the works of every period, a third describes every
re-dating.

Reading, sorting (passages.read_matches / sort_records), the metadata join (groups.read_meta /
keys_of), the periods, the unit map and writing are host plumbing; the passages, the unit x
work incidence matrix, the re-datings, the unit x re-dating product of the period offsets and the
sweeps come from the GPU (fs_trends), the regions from fs_quotes.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import n_script_of, prefixed, run, script_labels, work_names
from .companions import units_of, word_units_of
from .contrast import active_works
from .groups import NO_METADATA, UNKNOWN_DATE, keys_of, read_meta, stem
from .passages import sort_records
from .quotes import word_labels

BY = ('year', 'month')
UNIT = ('region', 'word', 'scene', 'character')
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE',
               'QUOTING_WORKS', 'FIRST_PERIOD', 'LAST_PERIOD', 'MEAN_PERIOD_MILLI',
               'POOL_MEAN_PERIOD_MILLI', 'SHIFT_MILLI', 'DIRECTION', 'STATISTIC', 'GE', 'P_PPM',
               'ADJ_GE', 'ADJ_PPM', 'TEXT']
PERIOD_FIELDS = ['PERIOD', 'OFFSET', 'WORKS', 'ACTIVE_WORKS']
PERMUTATION_FIELDS = ['PERMUTATION', 'POOL_OFFSET_SUM', 'MAX_STATISTIC', 'MAX_UNIT']


def find_trends(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, when, min_words=6,
                max_gap=0, min_quoting=5, permutations=1000, seed=0, device=0, sums=False):
    """(abi.TRENDS_UNIT_DTYPE[n_units], abi.TRENDS_PERM_DTYPE[permutations]) of records sorted
    by (work, fan_ix), the unit (or abi.FS_NONE) of each of the n_script words and the period
    offset of each of the n_works works (below 1024, or abi.TRENDS_OUT outside the pool); with
    `sums` a third array, uint32 [n_units][permutations], the offsets of every re-dating summed
    over the works quoting a unit."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    when = np.ascontiguousarray(when, dtype=np.uint16)
    n, n_units, permutations = len(work), int(n_units), int(permutations)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    if len(when) != int(n_works):
        raise ValueError("%d period offsets for %d works" % (len(when), n_works))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("a seed outside 0 .. 2^64 - 1")
    units = np.zeros(n_units, dtype=abi.TRENDS_UNIT_DTYPE)
    perms = np.zeros(max(0, permutations), dtype=abi.TRENDS_PERM_DTYPE)
    table = np.zeros((n_units, max(0, permutations)), dtype=np.uint32) if sums else None
    _lib.check(_lib.load().fs_trends(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), when.ctypes.data_as(C.c_void_p),
        int(min_quoting), permutations, int(seed), units.ctypes.data_as(C.c_void_p),
        perms.ctypes.data_as(C.c_void_p),
        table.ctypes.data_as(C.c_void_p) if sums else None), "fs_trends")
    return (units, perms, table) if sums else (units, perms)


def check_by(by):
    if by not in BY:
        raise ValueError("--by takes year or month, not %r" % (by,))


def number_of(key):
    """The number of a period key of groups.keys_of: YYYY for a year, YYYY * 12 + MM - 1 for a
    month YYYY-MM."""
    return int(key) if len(key) == 4 else int(key[:4]) * 12 + int(key[5:7]) - 1


def label_of(number, by):
    """The key of a period number."""
    return '%04d' % number if by == 'year' else '%04d-%02d' % (number // 12, number % 12 + 1)


def periods_of(names, meta, by):
    """(when[len(names)] as uint16: the period offset x(w), or abi.TRENDS_OUT for a work
    without metadata or without a date; base, the smallest period number; the key of every
    work) for the works `names` of a match file and read_meta's rows.  ValueError for two works
    of one file stem, an empty pool, a pool of one period and a span above 1023."""
    check_by(by)
    seen = {}
    for name in names:
        if seen.setdefault(stem(name), name) != name:
            raise ValueError("the works %r and %r of the match file are one work, %r"
                             % (seen[stem(name)], name, stem(name)))
    keys = [keys_of(meta[stem(n)], by)[0] if stem(n) in meta else NO_METADATA for n in names]
    numbers = [None if k in (UNKNOWN_DATE, NO_METADATA) else number_of(k) for k in keys]
    dated = [x for x in numbers if x is not None]
    if not dated:
        raise ValueError("the pool is empty: no work of the match file has a publication date")
    base, last = min(dated), max(dated)
    if last == base:
        raise ValueError("every dated work of the match file is of the %s %s: a trend needs two "
                         "periods" % (by, label_of(base, by)))
    if last - base >= abi.FS_TRENDS_MAX_SPAN:
        raise ValueError("the %ss from %s to %s span %d periods, more than %d"
                         % (by, label_of(base, by), label_of(last, by), last - base,
                            abi.FS_TRENDS_MAX_SPAN - 1))
    when = np.array([abi.TRENDS_OUT if x is None else x - base for x in numbers], dtype=np.uint16)
    return when, base, keys


def tables(rows, meta, by='year', unit='region', min_words=6, max_gap=0, min_works=1,
           min_quoting=5, permutations=1000, seed=0, device=0):
    """(units, periods, permutations): the three CSVs' rows, without headers, for the records
    `rows` (read_matches) and the metadata rows `meta` (read_meta)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), meta, by,
                   unit, min_words, max_gap, min_works, min_quoting, permutations, seed, device)


def tables_device(mf, meta, by='year', unit='region', min_words=6, max_gap=0, min_works=1,
                  min_quoting=5, permutations=1000, seed=0, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, meta, by, unit,
                   min_words, max_gap, min_works, min_quoting, permutations, seed, device)


def _tables(labels, names, work, fan, orig, comb, n_script, meta, by, unit, min_words, max_gap,
            min_works, min_quoting, permutations, seed, device):
    if unit not in UNIT:
        raise ValueError("--unit %r: region, word, scene or character" % (unit,))
    if not len(work):                               # a file without records: three header rows
        return [], [], []
    when, base, keys = periods_of(names, meta, by)
    if unit == 'word':
        unit_of, about = word_units_of(labels, work, fan, orig, comb, len(names), n_script,
                                       min_words, max_gap, min_works, device)
    else:
        unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, unit,
                                  min_words, max_gap, min_works, device)
    units, perms = find_trends(work, fan, orig, len(names), n_script, unit_of, len(about), when,
                               min_words, max_gap, min_quoting, permutations, seed, device)
    active = active_works(work, fan, orig, len(names), min_words, max_gap, device)
    pool = when[when != abi.TRENDS_OUT].astype(np.int64)
    n, big_x, P = len(pool), int(pool.sum()), int(permutations)
    family = [u for u in range(len(about)) if int(units[u]['adj_ge']) != abi.FS_NONE]
    family.sort(key=lambda u: (int(units[u]['adj_ge']), -int(units[u]['statistic']), u))
    utab = []
    for u in family:
        v = units[u]
        t, s, d = int(v['quoting']), int(v['offset_sum']), int(v['d'])
        ge, adj = int(v['ge']), int(v['adj_ge'])
        utab.append([u + 1] + list(about[u][:4])
                    + [t, label_of(base + int(v['first_x']), by),
                       label_of(base + int(v['last_x']), by), base * 1000 + s * 1000 // t,
                       base * 1000 + big_x * 1000 // n, abs(d) * 1000 // (t * n),
                       'later' if d > 0 else 'earlier' if d < 0 else '=', int(v['statistic']),
                       ge, (ge + 1) * 1000000 // (P + 1), adj, (adj + 1) * 1000000 // (P + 1),
                       about[u][4]])
    dtab = []
    for x in range(int(pool.max()) + 1):
        mine = when == x
        dtab.append([label_of(base + x, by), x, int(mine.sum()), int((mine & active).sum())])
    for key in (UNKNOWN_DATE, NO_METADATA):
        mine = np.array([k == key for k in keys], dtype=bool)
        dtab.append([key, '', int(mine.sum()), int((mine & active).sum())])
    ptab = [[r + 1, int(p['offset_sum']), int(p['max_statistic']),
             '' if int(p['max_unit']) == abi.FS_NONE else int(p['max_unit']) + 1]
            for r, p in enumerate(perms)]
    return utab, dtab, ptab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-trends.csv', '-trends-periods.csv', '-trends-permutations.csv'))


def process(args):
    """`ao3.py trends matches meta [--by year|month] [-o PREFIX]
    [--unit region|word|scene|character] [--min-words M] [--max-gap G] [--min-works K]
    [--min-quoting Q] [--permutations P] [--seed S] [--device D] [--reader {device,python}]`."""
    check_by(args.by)
    meta = read_meta(args.meta, args.by)            # (small: always read on the host)
    for row in meta.values():
        keys_of(row, args.by)                       # (a malformed row stops before the GPU)
    opts = (meta, args.by, args.unit, args.min_words, args.max_gap, args.min_works,
            args.min_quoting, args.permutations, args.seed, args.device)
    return run(args, (UNIT_FIELDS, PERIOD_FIELDS, PERMUTATION_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
