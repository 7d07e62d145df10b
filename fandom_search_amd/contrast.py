"""`ao3.py contrast`: what one group of fan works quotes more than another.

`groups` counts the works of every group per script word and leaves two columns of counts with
nothing to judge them by; among the thousands of words and hundreds of regions of a script a
twentieth of all differences looks significant at the usual level by accident.  This command
takes two disjoint sets of works, A and B, by the metadata keys of `groups` (`--by`, `--a`,
`--b`), and for every unit (a region of `quotes`, a script word inside one, a scene or a
character) prints the share of either side quoting it, how often a random relabelling of the
same works gives a difference at least as large, and how often the largest standardised
difference over all units of a relabelling is as large: one permutation test with the
max-statistic correction, which keeps the units' correlation through the works that quote
several of them.  A second file describes the sides, a third every permutation.

Reading, sorting (passages.read_matches / sort_records), the metadata join (groups.read_meta /
keys_of), the unit map and writing are host plumbing; the passages, the unit x work incidence
matrix, the selection of every permutation's side A, the unit x permutation product and the
sweeps come from the GPU (fs_contrast), the regions from fs_quotes.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import n_script_of, prefixed, run, script_labels, work_names
from .companions import units_of, word_units_of
from .groups import NO_METADATA, keys_of, read_meta, stem
from .passages import find_passages, sort_records
from .quotes import word_labels

UNIT = ('region', 'word', 'scene', 'character')
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'A_WORKS',
               'B_WORKS', 'A_PPM', 'B_PPM', 'EXPECTED_A_MILLI', 'DIRECTION', 'RATIO_PERMILLE',
               'STATISTIC', 'GE', 'P_PPM', 'ADJ_GE', 'ADJ_PPM', 'TEXT']
SIDE_FIELDS = ['SIDE', 'KEYS', 'WORKS', 'ACTIVE_WORKS', 'UNITS_QUOTED']
PERMUTATION_FIELDS = ['PERMUTATION', 'A_ACTIVE_WORKS', 'MAX_STATISTIC', 'MAX_UNIT']
EVERY_OTHER = '(every other work)'


def find_contrast(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, side, min_words=6,
                  max_gap=0, min_quoting=5, permutations=1000, seed=0, key_bits=32, device=0,
                  a_counts=False):
    """(abi.CONTRAST_UNIT_DTYPE[n_units], abi.CONTRAST_PERM_DTYPE[permutations]) of records
    sorted by (work, fan_ix), the unit (or abi.FS_NONE) of each of the n_script words and the
    side byte of each of the n_works works (0 out, 1 A, 2 B); with `a_counts` a third array,
    uint32 [n_units][permutations], the works of every permutation's side A quoting a unit."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    side = np.ascontiguousarray(side, dtype=np.uint8)
    n, n_units, permutations = len(work), int(n_units), int(permutations)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    if len(side) != int(n_works):
        raise ValueError("%d side bytes for %d works" % (len(side), n_works))
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError("a seed outside 0 .. 2^64 - 1")
    units = np.zeros(n_units, dtype=abi.CONTRAST_UNIT_DTYPE)
    perms = np.zeros(max(0, permutations), dtype=abi.CONTRAST_PERM_DTYPE)
    counts = np.zeros((n_units, max(0, permutations)), dtype=np.uint32) if a_counts else None
    _lib.check(_lib.load().fs_contrast(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), side.ctypes.data_as(C.c_void_p),
        int(min_quoting), permutations, int(seed), int(key_bits),
        units.ctypes.data_as(C.c_void_p), perms.ctypes.data_as(C.c_void_p),
        counts.ctypes.data_as(C.c_void_p) if a_counts else None), "fs_contrast")
    return (units, perms, counts) if a_counts else (units, perms)


def matching(names, meta, by, keys):
    """Per work of `names` whether one of its keys (groups.keys_of; a work without a metadata
    row has the key `(no metadata)`) is in `keys`."""
    keys = set(keys)
    return [not keys.isdisjoint(keys_of(meta[stem(n)], by) if stem(n) in meta else [NO_METADATA])
            for n in names]


def sides_of(names, meta, by, a_keys, b_keys):
    """(side[len(names)] as uint8: 0 out, 1 A, 2 B; (NA, NB, BOTH, OUT)) for the works `names`
    of a match file and read_meta's rows.  Without b_keys side B is every work that does not
    match A; with them a work matching both lists is on neither side.  ValueError for an empty
    side, and for two works of one file stem."""
    seen = {}
    for name in names:
        if seen.setdefault(stem(name), name) != name:
            raise ValueError("the works %r and %r of the match file are one work, %r"
                             % (seen[stem(name)], name, stem(name)))
    in_a = matching(names, meta, by, a_keys)
    in_b = matching(names, meta, by, b_keys) if b_keys else [not x for x in in_a]
    side = np.array([0 if a == b else 1 if a else 2 for a, b in zip(in_a, in_b)], dtype=np.uint8)
    counts = (int((side == 1).sum()), int((side == 2).sum()),
              sum(1 for a, b in zip(in_a, in_b) if a and b),
              sum(1 for a, b in zip(in_a, in_b) if not a and not b))
    for label, n in zip('AB', counts):
        if not n:
            raise ValueError("side %s is empty: no work of the match file has one of its keys"
                             % label)
    return side, counts


def active_works(work, fan_ix, orig_ix, n_works, min_words=6, max_gap=0, device=0):
    """bool[n_works]: the works with a passage (fs_passages)."""
    none = np.zeros(len(work), dtype=np.float64)
    found = find_passages(work, fan_ix, orig_ix, none, none, min_words, max_gap, device)
    active = np.zeros(int(n_works), dtype=bool)
    active[abi.as_u32(work)[found['first'].astype(np.int64)]] = True
    return active


def tables(rows, meta, by='year', a_keys=(), b_keys=(), unit='region', min_words=6, max_gap=0,
           min_works=1, min_quoting=5, permutations=1000, seed=0, device=0):
    """(units, sides, permutations): the three CSVs' rows, without headers, for the records
    `rows` (read_matches) and the metadata rows `meta` (read_meta)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), meta, by,
                   a_keys, b_keys, unit, min_words, max_gap, min_works, min_quoting, permutations,
                   seed, device)


def tables_device(mf, meta, by='year', a_keys=(), b_keys=(), unit='region', min_words=6,
                  max_gap=0, min_works=1, min_quoting=5, permutations=1000, seed=0, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, meta, by, a_keys,
                   b_keys, unit, min_words, max_gap, min_works, min_quoting, permutations, seed,
                   device)


def _tables(labels, names, work, fan, orig, comb, n_script, meta, by, a_keys, b_keys, unit,
            min_words, max_gap, min_works, min_quoting, permutations, seed, device):
    if unit not in UNIT:
        raise ValueError("--unit %r: region, word, scene or character" % (unit,))
    if not len(work):                               # a file without records: three header rows
        return [], [], []
    side, (na, nb, both, out) = sides_of(names, meta, by, a_keys, b_keys)
    if unit == 'word':
        unit_of, about = word_units_of(labels, work, fan, orig, comb, len(names), n_script,
                                       min_words, max_gap, min_works, device)
    else:
        unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, unit,
                                  min_words, max_gap, min_works, device)
    units, perms = find_contrast(work, fan, orig, len(names), n_script, unit_of, len(about), side,
                                 min_words, max_gap, min_quoting, permutations, seed, 32, device)
    active = active_works(work, fan, orig, len(names), min_words, max_gap, device)
    n, P = na + nb, int(permutations)
    family = [u for u in range(len(about)) if int(units[u]['adj_ge']) != abi.FS_NONE]
    family.sort(key=lambda u: (int(units[u]['adj_ge']), -int(units[u]['statistic']), u))
    utab = []
    for u in family:
        v = units[u]
        a, b, d = int(v['a_works']), int(v['b_works']), int(v['d'])
        appm, bppm = a * 1000000 // na, b * 1000000 // nb
        lo, hi = min(appm, bppm), max(appm, bppm)
        ge, adj = int(v['ge']), int(v['adj_ge'])
        utab.append([u + 1] + list(about[u][:4])
                    + [a, b, appm, bppm, (a + b) * na * 1000 // n,
                       'A' if d > 0 else 'B' if d < 0 else '=', hi * 1000 // lo if lo else '',
                       int(v['statistic']), ge, (ge + 1) * 1000000 // (P + 1), adj,
                       (adj + 1) * 1000000 // (P + 1), about[u][4]])
    in_a = np.array(matching(names, meta, by, a_keys), dtype=bool)
    stab = [['A', '; '.join(a_keys), na, int((active & (side == 1)).sum()),
             sum(1 for u in family if units[u]['a_works'])],
            ['B', '; '.join(b_keys) if b_keys else EVERY_OTHER, nb,
             int((active & (side == 2)).sum()), sum(1 for u in family if units[u]['b_works'])],
            ['BOTH', '', both, int((active & (side == 0) & in_a).sum()), ''],
            ['OUT', '', out, int((active & (side == 0) & ~in_a).sum()), '']]
    ptab = [[r + 1, int(p['a_active']), int(p['max_statistic']),
             '' if int(p['max_unit']) == abi.FS_NONE else int(p['max_unit']) + 1]
            for r, p in enumerate(perms)]
    return utab, stab, ptab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-contrast.csv', '-contrast-sides.csv', '-contrast-permutations.csv'))


def process(args):
    """`ao3.py contrast matches meta --a KEY [--a KEY ...] [--b KEY ...] [--by B] [-o PREFIX]
    [--unit region|word|scene|character] [--min-words M] [--max-gap G] [--min-works K]
    [--min-quoting Q] [--permutations P] [--seed S] [--device D] [--reader {device,python}]`."""
    meta = read_meta(args.meta, args.by)            # (small: always read on the host)
    for row in meta.values():
        keys_of(row, args.by)                       # (a malformed row stops before the GPU)
    opts = (meta, args.by, tuple(args.a), tuple(args.b or ()), args.unit, args.min_words,
            args.max_gap, args.min_works, args.min_quoting, args.permutations, args.seed,
            args.device)
    return run(args, (UNIT_FIELDS, SIDE_FIELDS, PERMUTATION_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
