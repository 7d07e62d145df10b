"""`ao3.py works`: the per-word match records of a search summarised by fan work.

`format` counts reuse per script word, `matrix` one n-gram per span, `passages` lists every
span.  This command answers which fan works reuse the script, how much of it, and which scenes
and characters they take it from: one row per work (matched and exact words, the cumulative
distance counts of `format`, distinct script words, passage statistics, scenes and characters
touched and the top one of each) and the work x scene and work x character matrices without
their zeros.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
reduction by work runs on the GPU (fs_works), once with the scene of every script word as its
group and once with its character.  Scene and character labels come from the records: a label's
id is its rank by the smallest ORIGINAL_SCRIPT_WORD_INDEX it occurs at (script order).
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, work_names
from .format import THRESHOLDS, THRESHOLD_NAMES
from .passages import _CHAR, _SCENE, sort_records

WORK_FIELDS = (['FAN_WORK_FILENAME', 'MATCHED_WORDS', 'EXACT_WORDS'] + THRESHOLD_NAMES +
               ['DISTINCT_SCRIPT_WORDS', 'PASSAGES', 'PASSAGE_WORDS', 'LONGEST_PASSAGE',
                'FAN_WORK_WORD_FIRST', 'FAN_WORK_WORD_LAST',
                'SCENES', 'TOP_SCENE', 'TOP_SCENE_WORDS',
                'CHARACTERS', 'TOP_CHARACTER', 'TOP_CHARACTER_WORDS'])
SCENE_FIELDS = ['FAN_WORK_FILENAME', 'ORIGINAL_SCRIPT_SCENE', 'MATCHED_WORDS', 'EXACT_WORDS']
CHARACTER_FIELDS = ['FAN_WORK_FILENAME', 'ORIGINAL_SCRIPT_CHARACTER', 'MATCHED_WORDS',
                    'EXACT_WORDS']


def summarise(work, fan_ix, orig_ix, comb, n_works, n_script, group_of=None, n_groups=0,
              min_words=6, max_gap=0, thresholds=THRESHOLDS, device=0):
    """(abi.WORK_DTYPE[n_works], counts[n_works][len(thresholds) + 1], abi.WORK_CELL_DTYPE
    cells sorted by (work, group)) of records sorted by (work, fan_ix); `group_of`: group id
    < n_groups of every script word, or None."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    comb = np.ascontiguousarray(comb, dtype=np.float64)
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    n, n_works, n_groups = len(work), int(n_works), int(n_groups)
    if not (len(fan) == len(orig) == len(comb) == n):
        raise ValueError("columns of different lengths")
    gmap = None
    if group_of is not None:
        gmap = abi.as_u32(group_of)
        if len(gmap) != int(n_script):
            raise ValueError("group_of needs one entry per script word")
    elif n_groups:
        raise ValueError("n_groups without group_of")
    L = _lib.load()
    out = np.zeros(n_works, dtype=abi.WORK_DTYPE)
    counts = np.zeros((n_works, len(thr) + 1), dtype=np.uint32)
    most = min(n, n_works * n_groups)               # a record makes at most one cell
    cells = grow(lambda cells, cap, got: L.fs_works(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(comb, C.c_double), n, n_works, int(n_script),
        abi.ptr(gmap, C.c_uint32), n_groups, int(min_words), int(max_gap),
        abi.ptr(thr, C.c_double), len(thr), out.ctypes.data_as(C.c_void_p),
        counts.ctypes.data_as(C.c_void_p), cells, cap, got),
        abi.WORK_CELL_DTYPE, min(most, max(4096, n // 8)), "fs_works")
    return out, counts, cells


def label_groups(orig, labels, what):
    """(group_of[n_script], names): the labels numbered by the smallest script word index they
    occur at; script words without a record get group 0.  ValueError for a script word that
    carries two labels."""
    label_at = {}
    for o, lab in zip(orig.tolist(), labels):
        if label_at.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two %ss, %r and %r: records of different "
                             "scripts in one file?" % (o, what, label_at[o], lab))
    return groups_of_labels(label_at, n_script_of(orig))


def groups_of_labels(label_at, n_script):
    """label_groups' result for {script word: label}."""
    ids, names = {}, []
    group_of = np.zeros(n_script, dtype=np.uint32)
    for o in sorted(label_at):
        lab = label_at[o]
        if lab not in ids:
            ids[lab] = len(names)
            names.append(lab)
        group_of[o] = ids[lab]
    return group_of, names


def tables(rows, min_words=6, max_gap=0, device=0):
    """(works, scenes, characters): the three CSVs' rows, without headers, for the records
    `rows` (read_matches)."""
    order, work, fan, orig, _, comb = sort_records(rows)
    srt = [rows[i] for i in order]
    groups = [label_groups(orig, [r[col] for r in srt], what)
              for col, what in ((_SCENE, 'scene'), (_CHAR, 'character'))]
    return _tables(work_names(rows), work, fan, orig, comb, n_script_of(orig), groups, min_words,
                   max_gap, device)


def tables_device(mf, min_words=6, max_gap=0, device=0):
    """tables over a matches.MatchFile, one label decoded per script word; None when a script
    word's records spell a label in two ways (tables() then says what is wrong, or finds the
    two spellings equal)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    groups = []
    for col in (_SCENE, _CHAR):
        label_at = mf.labels(col, n_script)
        if label_at is None:
            return None
        groups.append(groups_of_labels(label_at, n_script))
    return _tables(mf.names, work, fan, orig, comb, n_script, groups, min_words, max_gap, device)


def _tables(names, work, fan, orig, comb, n_script, groups, min_words, max_gap, device):
    res = []
    for group_of, labels in groups:
        res.append((labels,) + summarise(work, fan, orig, comb, len(names), n_script, group_of,
                                         len(labels), min_words, max_gap, THRESHOLDS, device))
    (scenes, ws, counts, scells), (chars, wc, _, ccells) = res
    table = []
    for w, name in enumerate(names):
        a, b = ws[w], wc[w]
        table.append([name, int(a['n_words']), int(counts[w][0])] +
                     [int(c) for c in counts[w][:len(THRESHOLDS)]] +
                     [int(a['n_script_words']), int(a['n_passages']), int(a['passage_words']),
                      int(a['longest']), int(a['fan_first']), int(a['fan_last']),
                      int(a['n_groups_hit']), scenes[int(a['top_group'])],
                      int(a['top_group_words']),
                      int(b['n_groups_hit']), chars[int(b['top_group'])],
                      int(b['top_group_words'])])
    out = [table]
    for labels, cells in ((scenes, scells), (chars, ccells)):
        out.append([[names[int(c['work'])], labels[int(c['group'])], int(c['n_words']),
                     int(c['n_exact'])] for c in cells])
    return tuple(out)


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-works.csv', '-works-scenes.csv', '-works-characters.csv'))


def process(args):
    """`ao3.py works matches [-o PREFIX] [--min-words M] [--max-gap G] [--device D]
    [--reader {device,python}]`."""
    return run(args, (WORK_FIELDS, SCENE_FIELDS, CHARACTER_FIELDS),
               output_names(args.matches, args.output), tables, tables_device,
               (args.min_words, args.max_gap, args.device))
