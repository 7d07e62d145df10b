"""`ao3.py transitions`: after fans quote this stretch of the script, which stretch do they quote
next?

`companions` relates two stretches by the works that quote both and cannot tell "scene 12 then
scene 13" from the reverse; `retellings` knows the order but keeps it inside one work.  This
command adds the order up over the corpus.  A unit is a region of `quotes` (`--by region`), a
scene or a character of the script; a passage belongs to the unit of its first script word, and
a work's passages that have a unit, in the order the work quotes them, are its sequence.  Two
neighbours of a sequence with at most `--within` fan words between them are a step from the
unit of the first to the unit of the second.  Per cell (from, to): its steps, how many of them
advance in the script, the works taking it; the cells with at least `--min-steps` steps of at
least `--min-step-works` works, making up at least `--min-share` percent of the steps leaving
`from`, are listed, ranked by steps.  Per unit: its passages and works, the works that open and
close on it, its steps out and in and its most usual successor.

Reading, sorting (passages.read_matches / sort_records), the unit map (companions.units_of) and
writing are host plumbing; the passages, the sequences, the steps and every count come from the
GPU (fs_transitions), the regions from fs_quotes.  A passage is what `passages` keeps under the
same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .companions import BY, units_of
from .passages import sort_records
from .quotes import word_labels

ANY = abi.FS_NONE       # --within: any distance
CELL_FIELDS = ['FROM', 'TO', 'FROM_FIRST_WORD_INDEX', 'FROM_LAST_WORD_INDEX', 'FROM_CHARACTER',
               'FROM_SCENE', 'TO_FIRST_WORD_INDEX', 'TO_LAST_WORD_INDEX', 'TO_CHARACTER',
               'TO_SCENE', 'STEPS', 'ADVANCES', 'WORKS', 'SHARE_PERCENT', 'LIFT_PERMILLE',
               'DIRECTION', 'FIRST_FAN_WORK_FILENAME', 'FROM_TEXT', 'TO_TEXT']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'PASSAGES',
               'WORKS', 'STARTS', 'ENDS', 'STEPS_OUT', 'STEPS_IN', 'SUCCESSORS', 'PREDECESSORS',
               'BEST_NEXT', 'BEST_NEXT_STEPS', 'TEXT']


def find_transitions(work, fan_ix, orig_ix, n_works, n_script, unit_of, n_units, min_words=6,
                     max_gap=0, within=ANY, min_steps=1, min_step_works=2, min_share=0, device=0):
    """(abi.TRANSITION_UNIT_DTYPE[n_units], abi.TRANSITION_DTYPE cells in (a, b) order) of
    records sorted by (work, fan_ix) and the unit (or abi.FS_NONE) of each of the n_script
    words."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    unit_of = abi.as_u32(unit_of)
    n, n_units = len(work), int(n_units)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    if len(unit_of) != int(n_script):
        raise ValueError("a unit map of %d entries for %d script words" % (len(unit_of), n_script))
    L = _lib.load()
    units = np.zeros(n_units, dtype=abi.TRANSITION_UNIT_DTYPE)
    cells = grow(lambda out, cap, got: L.fs_transitions(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), abi.ptr(unit_of, C.c_uint32),
        n_units, int(min_words), int(max_gap), int(within), int(min_steps), int(min_step_works),
        int(min_share), units.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.TRANSITION_DTYPE, 4096, "fs_transitions")
    return units, cells


def share_percent(steps, steps_out):
    return int(steps) * 100 // int(steps_out)


def lift_permille(steps, total_steps, steps_out, steps_in):
    """steps against what choosing the next stretch independently of the current one would
    give (1000), in Python ints: the products pass 2^64."""
    return int(steps) * int(total_steps) * 1000 // (int(steps_out) * int(steps_in))


def tables(rows, by='region', min_words=6, max_gap=0, min_works=1, within=ANY, min_steps=1,
           min_step_works=2, min_share=0, device=0):
    """(cells, units): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), by,
                   min_words, max_gap, min_works, within, min_steps, min_step_works, min_share,
                   device)


def tables_device(mf, by='region', min_words=6, max_gap=0, min_works=1, within=ANY, min_steps=1,
                  min_step_works=2, min_share=0, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, by, min_words,
                   max_gap, min_works, within, min_steps, min_step_works, min_share, device)


def _tables(labels, names, work, fan, orig, comb, n_script, by, min_words, max_gap, min_works,
            within, min_steps, min_step_works, min_share, device):
    if by not in BY:
        raise ValueError("--by %r: region, scene or character" % (by,))
    unit_of, about = units_of(labels, work, fan, orig, comb, len(names), n_script, by, min_words,
                              max_gap, min_works, device)
    units, cells = find_transitions(work, fan, orig, len(names), n_script, unit_of, len(about),
                                    min_words, max_gap, within, min_steps, min_step_works,
                                    min_share, device)
    return _rows_of(units, cells, about, names)


def _rows_of(units, cells, about, names):
    total = sum(int(v) for v in units['steps_out'])
    # STEPS descending, then FROM, then TO (the device's order, kept by a stable sort)
    order = np.argsort(-cells['steps'].astype(np.int64), kind='stable')
    ctab = []
    for c in cells[order]:
        a, b, n = int(c['a']), int(c['b']), int(c['steps'])
        ctab.append([a + 1, b + 1] + list(about[a][:4]) + list(about[b][:4])
                    + [n, int(c['advances']), int(c['works']),
                       share_percent(n, c['steps_out_a']),
                       lift_permille(n, total, c['steps_out_a'], c['steps_in_b']),
                       'forward' if b > a else 'back' if b < a else 'same',
                       names[int(c['first_work'])], about[a][4], about[b][4]])
    utab = []
    for u, v in enumerate(units):
        best = int(v['best_next'])
        utab.append([u + 1] + list(about[u][:4])
                    + [int(v[k]) for k in abi.TRANSITION_UNIT_DTYPE.names[:8]]
                    + ['' if best == abi.FS_NONE else best + 1, int(v['best_steps']),
                       about[u][4]])
    return ctab, utab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-transitions.csv', '-transitions-units.csv'))


def process(args):
    """`ao3.py transitions matches [-o PREFIX] [--by region|scene|character] [--min-words M]
    [--max-gap G] [--min-works K] [--within W] [--min-steps S] [--min-step-works N]
    [--min-share P] [--device D] [--reader {device,python}]`."""
    within = ANY if args.within is None else args.within
    opts = (args.by, args.min_words, args.max_gap, args.min_works, within, args.min_steps,
            args.min_step_works, args.min_share, args.device)
    return run(args, (CELL_FIELDS, UNIT_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
