"""`ao3.py misquotes`: the works that share departures from the script.

`pairs`, `clusters` and `neighbours` relate two works by the script words both quote, and two
works that both quote a famous line are close under that measure whether or not one ever saw
the other.  Shared *errors* are evidence of descent: two works that both write "Luke, I am your
father" did not each mishear the film the same way.  Here a departure is a record inside a
passage whose fan word is not the script word, a misquote a (script word, fan spelling) with a
departure, and a misquote that at most `--max-share` percent of the works quoting the word share
is telling: a spelling most of them share is a common reading (a line the transcript gets wrong,
a meme), not evidence of a particular link.  A telling misquote weighs the more the fewer of the
word's readers share it (`--weight rarity`: the bits of readers // works; `--weight flat`: 1).
Two works are scored by the telling misquotes both have; per kept pair the strongest shared
misquote and how much of the departures either makes, on ground both quote, the two have in
common.

Reading, sorting (passages.read_matches / sort_records), numbering the spellings
(variants.merge_spellings over fs_matches_intern's ids or a dict) and writing are host plumbing;
the passages, the sets, the numbering of the misquotes, the postings, their expansion into
pairs and the details of the kept pairs come from the GPU (fs_misquotes).  A passage is what
`passages` keeps under the same `--min-words` and `--max-gap`.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import _FAN_WORD, sort_records
from .quotes import word_labels
from .variants import fold_key, merge_spellings

WEIGHT = ('rarity', 'flat')
MISQUOTE_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD',
                   'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'FAN_WORK_WORD', 'RECORDS',
                   'WORKS', 'READERS', 'SHARE_PERCENT', 'TELLING', 'WEIGHT', 'PAIRS',
                   'FIRST_FAN_WORK_FILENAME']
PAIR_FIELDS = ['FAN_WORK_FILENAME_A', 'FAN_WORK_FILENAME_B', 'SHARED', 'SCORE', 'A_TELLING',
               'B_TELLING', 'A_ON_COMMON', 'B_ON_COMMON', 'AGREEMENT_PERCENT',
               'STRONGEST_SCRIPT_WORD_INDEX', 'STRONGEST_SCRIPT_WORD', 'STRONGEST_FAN_WORK_WORD',
               'STRONGEST_WORKS', 'STRONGEST_WEIGHT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'PASSAGE_RECORDS', 'DEPARTURES', 'MISQUOTES', 'TELLING',
               'SINGULAR', 'PARTNERS', 'CLOSEST', 'CLOSEST_SCORE']


def weight_code(weight):
    if weight not in WEIGHT:
        raise ValueError("--weight %r: rarity or flat" % (weight,))
    return abi.FS_MISQUOTES_FLAT if weight == 'flat' else abi.FS_MISQUOTES_RARITY


def find_misquotes(work, fan_ix, orig_ix, spell, same, n_works, n_spell, min_words=6, max_gap=0,
                   min_works=2, max_share=50, weight='rarity', min_shared=1, min_score=1,
                   device=0):
    """(abi.MISQUOTE_WORK_DTYPE[n_works], abi.MISQUOTE_DTYPE listed misquotes in the order of
    their numbers, abi.MISQUOTE_PAIR_DTYPE kept pairs in (a, b) order) of records sorted by
    (work, fan_ix); same[o]: the spelling that is script word o, abi.FS_NONE for none."""
    work, fan, orig, spell, same = (abi.as_u32(v) for v in (work, fan_ix, orig_ix, spell, same))
    n, n_works = len(work), int(n_works)
    if not (len(fan) == len(orig) == len(spell) == n):
        raise ValueError("columns of different lengths")
    code = weight_code(weight)
    L = _lib.load()
    works = np.zeros(n_works, dtype=abi.MISQUOTE_WORK_DTYPE)
    found, pairs = grow(lambda m, cap_m, got_m, p, cap_p, got_p: L.fs_misquotes(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(spell, C.c_uint32), abi.ptr(same, C.c_uint32), n,
        n_works, len(same), int(n_spell), int(min_words), int(max_gap), int(min_works),
        int(max_share), code, int(min_shared), int(min_score), works.ctypes.data_as(C.c_void_p),
        m, cap_m, got_m, p, cap_p, got_p),
        [abi.MISQUOTE_DTYPE, abi.MISQUOTE_PAIR_DTYPE], [1024, 4096], "fs_misquotes")
    return works, found, pairs


def same_spellings(labels, ids, n_script, fold_case):
    """same[o]: the id of the spelling that is script word o itself, abi.FS_NONE where no
    record's fan word is that spelling (or no record names o)."""
    same = np.full(n_script, abi.FS_NONE, dtype=np.uint32)
    for o, (word, _, _) in labels.items():
        same[o] = ids.get(fold_key(word, fold_case), abi.FS_NONE)
    return same


def tables(rows, min_words=6, max_gap=0, min_works=2, max_share=50, weight='rarity',
           min_shared=1, min_score=1, keep_case=False, device=0):
    """(misquotes, pairs, works): the three CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    order, work, fan, orig, _, _ = sort_records(rows)
    spell, ids, shown = merge_spellings([r[_FAN_WORD] for r in rows], not keep_case)
    return _tables(labels, work_names(rows), ids, shown, work, fan, orig, spell[order],
                   n_script_of(orig), min_words, max_gap, min_works, max_share, weight,
                   min_shared, min_score, keep_case, device)


def tables_device(mf, min_words=6, max_gap=0, min_works=2, max_share=50, weight='rarity',
                  min_shared=1, min_score=1, keep_case=False, device=0):
    """tables over a matches.MatchFile: the fan words numbered on the device, one text decoded
    per spelling and three labels per script word; None when a script word's records spell a
    label in two ways (tables() then decides)."""
    order, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    raw, first = mf.intern(_FAN_WORD)
    remap, ids, shown = merge_spellings(mf.text(_FAN_WORD, first), not keep_case)
    spell = np.take(remap, raw)[order] if mf.n else np.zeros(0, dtype=np.uint32)
    return _tables(labels, list(mf.names), ids, shown, work, fan, orig, spell, n_script,
                   min_words, max_gap, min_works, max_share, weight, min_shared, min_score,
                   keep_case, device)


def _tables(labels, names, ids, shown, work, fan, orig, spell, n_script, min_words, max_gap,
            min_works, max_share, weight, min_shared, min_score, keep_case, device):
    same = same_spellings(labels, ids, n_script, not keep_case)
    works, found, pairs = find_misquotes(work, fan, orig, spell, same, len(names), len(shown),
                                         min_words, max_gap, min_works, max_share, weight,
                                         min_shared, min_score, device)
    mtab = []
    for m in found.tolist():                                # the order of their numbers
        o, s, records, k, readers, telling, wt, first = m
        word, char, scene = labels[o]                       # a misquote has a record
        mtab.append([o, word, char, scene, shown[s], records, k, readers, k * 100 // readers,
                     telling, wt, k * (k - 1) // 2 if telling else 0, names[first]])
    # (a, b) order is the device's; one stable sort by score, then shared, both descending
    kept = pairs.tolist()
    kept.sort(key=lambda p: (-p[3], -p[2]))
    telling = works['telling'].tolist()
    ptab = []
    for a, b, shared, score, a_on, b_on, strong, strong_wt in kept:
        o, s, _, k = found[strong].tolist()[:4]
        ptab.append([names[a], names[b], shared, score, telling[a], telling[b], a_on, b_on,
                     shared * 100 // (a_on + b_on - shared), o, labels[o][0], shown[s], k,
                     strong_wt])
    wtab = []
    for w in np.flatnonzero(works['passage_records']).tolist():
        recs, dep, mis, tell, single, partners, closest, score = works[w].tolist()
        wtab.append([names[w], recs, dep, mis, tell, single, partners,
                     names[closest] if partners else '', score])
    return mtab, ptab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-misquotes.csv', '-misquotes-pairs.csv', '-misquotes-works.csv'))


def process(args):
    """`ao3.py misquotes matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-works W]
    [--max-share P] [--weight rarity|flat] [--min-shared S] [--min-score C] [--keep-case]
    [--device D] [--reader {device,python}]`."""
    weight_code(args.weight)
    opts = (args.min_words, args.max_gap, args.min_works, args.max_share, args.weight,
            args.min_shared, args.min_score, args.keep_case, args.device)
    return run(args, (MISQUOTE_FIELDS, PAIR_FIELDS, WORK_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
