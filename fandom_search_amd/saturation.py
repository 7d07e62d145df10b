"""`ao3.py saturation`: what a sample of the works would show.

A match file is a sample of a fandom, and no other command says whether it is large enough: had
a tenth of these works been scraped, how much of what fans quote would have been seen, and is the
curve still rising where the sample ends?  This command draws `--permutations` orders of the
works.  In order r work w arrives at time h(r, w), a pure function of (`--seed`, r, w); the
sample at fraction f is the works with h < f * 2^32, each work in it independently with
probability f, the samples nested as f grows.  At `--points` evenly spaced fractions it prints
how many units (script words inside a quoted region, regions, scenes or characters) the sample
has seen, as the `--level` percent interval, the median, the extremes and the mean over the
orders, beside the sample's size; per order where the curve passes half, nine tenths and all of
the quoted units; and a summary with the Chao2 lower bound of the quoted units not yet seen.

Reading, sorting (passages.read_matches / sort_records), the unit map, the Chao2 arithmetic and
writing are host plumbing; the passages, the unit x work incidence matrix, the first time of
every unit in every order (a min-product), the curves and the order statistics come from the
GPU (fs_saturation), the regions from fs_quotes.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import n_script_of, prefixed, run, script_labels, work_names
from .companions import units_of, word_units_of
from .passages import sort_records
from .quotes import word_labels

BY = ('region', 'word', 'scene', 'character')
POINT_FIELDS = ['POINT', 'SAMPLE_PPM', 'WORKS_LOW', 'WORKS_MEDIAN', 'WORKS_HIGH',
                'WORKS_MEAN_MILLI', 'UNITS_LOW', 'UNITS_MEDIAN', 'UNITS_HIGH', 'UNITS_MIN',
                'UNITS_MAX', 'UNITS_MEAN_MILLI', 'UNITS_PERCENT', 'NEW_PER_WORK_MILLI']
PERMUTATION_FIELDS = ['PERMUTATION', 'HALF_AT_PPM', 'NINETY_AT_PPM', 'ALL_AT_PPM']
SUMMARY_FIELDS = ['WORKS', 'ACTIVE_WORKS', 'UNITS', 'UNITS_QUOTED', 'QUOTED_BY_ONE',
                  'QUOTED_BY_TWO', 'UNSEEN_ESTIMATE', 'ESTIMATED_TOTAL', 'SEEN_PERCENT',
                  'HALF_AT_PPM', 'NINETY_AT_PPM', 'ALL_AT_PPM']


def find_saturation(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                    max_gap=0, permutations=1000, points=100, seed=0, level=95, first=False,
                    device=0):
    """(works uint32[n_units], abi.SATURATION_POINT_DTYPE[points],
    abi.SATURATION_PERM_DTYPE[permutations], abi.SATURATION_SUMMARY_DTYPE[1]) of records sorted
    by (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script words; with `first`
    a fifth array, uint32[n_units][permutations], the first time of every unit in every order."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units = len(work), int(n_units)
    permutations, points = int(permutations), int(points)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("a seed outside 0 .. 2^64 - 1")
    works = np.zeros(n_units, dtype=np.uint32)
    pts = np.zeros(max(0, points), dtype=abi.SATURATION_POINT_DTYPE)
    perms = np.zeros(max(0, permutations), dtype=abi.SATURATION_PERM_DTYPE)
    summary = np.zeros(1, dtype=abi.SATURATION_SUMMARY_DTYPE)
    times = np.zeros((n_units, max(0, permutations)), dtype=np.uint32) if first else None
    _lib.check(_lib.load().fs_saturation(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), permutations, points, int(seed), int(level),
        works.ctypes.data_as(C.c_void_p), pts.ctypes.data_as(C.c_void_p),
        perms.ctypes.data_as(C.c_void_p), summary.ctypes.data_as(C.c_void_p),
        times.ctypes.data_as(C.c_void_p) if first else None), "fs_saturation")
    return (works, pts, perms, summary) + ((times,) if first else ())


def unseen_estimate(n_works, q1, q2):
    """The bias-corrected Chao2 lower bound of the quoted units not yet seen, rounded down."""
    if n_works < 1:
        return 0
    return ((n_works - 1) * q1 * (q1 - 1)) // (n_works * 2 * (q2 + 1))


def tables(rows, by='word', min_words=6, max_gap=0, min_works=1, permutations=1000, points=100,
           seed=0, level=95, device=0):
    """(points, permutations, summary): the three CSVs' rows, without headers, for the records
    `rows` (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, permutations, points, seed, level, device)


def tables_device(mf, by='word', min_words=6, max_gap=0, min_works=1, permutations=1000,
                  points=100, seed=0, level=95, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, permutations, points, seed, level, device)


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            permutations, points, seed, level, device):
    if by not in BY:
        raise ValueError("--by %r: region, word, scene or character" % (by,))
    if not len(work):                               # a file without records: three header rows
        return [], [], []
    if by == 'word':
        unit_of, about = word_units_of(labels, work, fan, orig, comb, len(names), n_script,
                                       min_words, max_gap, min_works, device)
    else:
        unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by,
                                  min_words, max_gap, min_works, device)
    _, pts, perms, summary = find_saturation(work, fan, orig, len(names), n_script, unit_of,
                                             len(about), min_words, max_gap, permutations,
                                             points, seed, level, device=device)
    K, R = int(points), int(permutations)
    s = summary[0]
    Q, q1, q2 = int(s['units_quoted']), int(s['singletons']), int(s['doubletons'])

    def ppm(c):
        return int(c) * 1000000 // K
    ptab, usum0, wsum0 = [], 0, 0
    for c, p in enumerate(pts, 1):
        usum, wsum = int(p['units_sum']), int(p['works_sum'])
        ptab.append([c, ppm(c), int(p['works_low']), int(p['works_median']), int(p['works_high']),
                     wsum * 1000 // R, int(p['units_low']), int(p['units_median']),
                     int(p['units_high']), int(p['units_min']), int(p['units_max']),
                     usum * 1000 // R, int(p['units_median']) * 100 // max(1, Q),
                     (usum - usum0) * 1000 // max(1, wsum - wsum0)])
        usum0, wsum0 = usum, wsum
    rtab = [[r + 1, ppm(v['half_at']), ppm(v['ninety_at']), ppm(v['all_at'])]
            for r, v in enumerate(perms)]
    unseen = unseen_estimate(len(names), q1, q2)
    mid = (R - 1) // 2
    stab = [[len(names), int(s['n_active']), len(about), Q, q1, q2, unseen, Q + unseen,
             Q * 100 // max(1, Q + unseen)]
            + [ppm(sorted(perms[k].tolist())[mid]) for k in ('half_at', 'ninety_at', 'all_at')]]
    return ptab, rtab, stab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-saturation.csv', '-saturation-permutations.csv',
                                      '-saturation-summary.csv'))


def process(args):
    """`ao3.py saturation matches [-o PREFIX] [--by word|region|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--permutations R] [--points K] [--seed S] [--level L]
    [--device D] [--reader {device,python}]`."""
    opts = (args.by, args.min_words, args.max_gap, args.min_works, args.permutations,
            args.points, args.seed, args.level, args.device)
    return run(args, (POINT_FIELDS, PERMUTATION_FIELDS, SUMMARY_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
