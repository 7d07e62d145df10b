"""`ao3.py intervals`: how sure the works-per-stretch counts are.

`quotes`, `companions`, `lines` and `works` print counts of works; a match file is a sample of a
fandom, and none of them says which differences between two counts would survive another sample.
This command resamples the fan works: a Poisson bootstrap, in which every work counts m(b, w)
times in replicate b, a pure function of (`--seed`, b, w) distributed as Poisson(1).  Every unit
(a region of `quotes`, a script word inside one, a scene or a character) is recounted in every
replicate; the command prints per unit the `--level` percent interval and the median of its
count and of its share of the resampled works in parts per million, the mean, its rank, and in
how many replicates it stays ahead of the unit that follows it in the observed order.  A second
file says per replicate how many works were drawn and how many units anyone quoted.

Reading, sorting (passages.read_matches / sort_records), the unit map and writing are host
plumbing; the passages, the unit x work incidence matrix, the multiplicities, the unit x
replicate product (on the matrix cores) and the order statistics come from the GPU
(fs_intervals), the regions from fs_quotes.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import n_script_of, prefixed, run, script_labels, work_names
from .companions import units_of, word_units_of
from .passages import sort_records
from .quotes import word_labels

BY = ('region', 'word', 'scene', 'character')
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'WORKS_LOW', 'WORKS_MEDIAN', 'WORKS_HIGH', 'PPM', 'PPM_LOW', 'PPM_MEDIAN',
               'PPM_HIGH', 'MEAN_MILLI', 'RANK', 'NEXT', 'AHEAD_OF_NEXT', 'TIED_WITH_NEXT',
               'BEHIND_NEXT', 'TEXT']
REPLICATE_FIELDS = ['REPLICATE', 'RESAMPLED_WORKS', 'RESAMPLED_ACTIVE', 'UNITS_QUOTED']


def find_intervals(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                   max_gap=0, replicates=1000, seed=0, level=95, device=0):
    """(abi.INTERVAL_UNIT_DTYPE[n_units], abi.INTERVAL_REPLICATE_DTYPE[replicates]) of records
    sorted by (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script words."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units, replicates = len(work), int(n_units), int(replicates)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("a seed outside 0 .. 2^64 - 1")
    units = np.zeros(n_units, dtype=abi.INTERVAL_UNIT_DTYPE)
    reps = np.zeros(max(0, replicates), dtype=abi.INTERVAL_REPLICATE_DTYPE)
    _lib.check(_lib.load().fs_intervals(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), replicates, int(seed), int(level),
        units.ctypes.data_as(C.c_void_p), reps.ctypes.data_as(C.c_void_p)), "fs_intervals")
    return units, reps


def tables(rows, by='region', min_words=6, max_gap=0, min_works=1, replicates=1000, seed=0,
           level=95, device=0):
    """(units, replicates): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, replicates, seed, level, device)


def tables_device(mf, by='region', min_words=6, max_gap=0, min_works=1, replicates=1000, seed=0,
                  level=95, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, replicates, seed, level, device)


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            replicates, seed, level, device):
    if by not in BY:
        raise ValueError("--by %r: region, word, scene or character" % (by,))
    if not len(work):                               # a file without records: two header rows
        return [], []
    if by == 'word':
        unit_of, about = word_units_of(labels, work, fan, orig, comb, len(names), n_script,
                                       min_words, max_gap, min_works, device)
    else:
        unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by,
                                  min_words, max_gap, min_works, device)
    units, reps = find_intervals(work, fan, orig, len(names), n_script, unit_of, len(about),
                                 min_words, max_gap, replicates, seed, level, device)
    utab = []
    for u, v in enumerate(units):
        nxt = int(v['next'])
        against = ['', '', '', ''] if nxt == abi.FS_NONE else \
            [nxt + 1, int(v['ahead']), int(v['tied']), int(v['behind'])]
        utab.append([u + 1] + list(about[u][:4])
                    + [int(v[k]) for k in ('works', 'works_low', 'works_median', 'works_high',
                                           'ppm', 'ppm_low', 'ppm_median', 'ppm_high',
                                           'mean_milli', 'rank')]
                    + against + [about[u][4]])
    rtab = [[b + 1, int(r['resampled_works']), int(r['resampled_active']),
             int(r['units_quoted'])] for b, r in enumerate(reps)]
    return utab, rtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-intervals.csv', '-intervals-replicates.csv'))


def process(args):
    """`ao3.py intervals matches [-o PREFIX] [--by region|word|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--replicates B] [--seed S] [--level L] [--device D]
    [--reader {device,python}]`."""
    opts = (args.by, args.min_words, args.max_gap, args.min_works, args.replicates, args.seed,
            args.level, args.device)
    return run(args, (UNIT_FIELDS, REPLICATE_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
