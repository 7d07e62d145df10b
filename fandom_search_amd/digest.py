"""`ao3.py digest`: the fewest works that show what the fan works quote.

Every other analysis command counts, groups or relates; this one selects.  It is greedy maximum
coverage: the first pick is the work covering most of the script, every later pick the work that
adds most script words to what the picks so far cover, the earlier work on a tie, until the
picks show every word anyone quotes (or `--picks`, `--cover` or `--min-gain` says stop).  The
list of picks is a reading list, and its CUM_PERCENT column says how concentrated the quoting is.
A second file says of every work with a passage how much of it the picks show, after which pick
they show all of it, and which pick is most like it.  A work covers every script word from the
first record of one of its passages to the last, bridged words included; a passage is what
`passages` keeps under the same `--min-words` and `--max-gap`.

Reading, sorting (passages.read_matches / sort_records), the two bincounts and writing are host
plumbing; the passages, the coverage, the rounds and the per-work figures come from the GPU
(fs_digest).
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels

PICK_FIELDS = ['RANK', 'FAN_WORK_FILENAME', 'COVERED_WORDS', 'NEW_WORDS', 'NEW_RUNS',
               'LONGEST_NEW_FIRST_WORD_INDEX', 'LONGEST_NEW_LAST_WORD_INDEX', 'LONGEST_NEW_WORDS',
               'CHARACTER', 'SCENE', 'CUM_WORDS', 'CUM_PERCENT', 'SUBSUMED_WORKS',
               'CUM_SUBSUMED_WORKS', 'REPRESENTED_WORKS', 'LONGEST_NEW_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'COVERED_WORDS', 'PICK_RANK', 'IN_PICKS_WORDS',
               'IN_PICKS_PERCENT', 'SUBSUMED_AT', 'BEST_PICK', 'BEST_PICK_FILENAME',
               'BEST_PICK_SHARED']


def find_digest(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0, picks=0,
                cover=100, min_gain=1, device=0):
    """(abi.DIGEST_PICK_DTYPE picks in pick order, abi.DIGEST_WORK_DTYPE per active work, TOTAL)
    of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n = len(work)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    total = C.c_uint64(0)
    # neither the picks nor the active works are more than the works: no second call
    room = max(1, min(int(n_works), n))
    found, works = grow(lambda p_out, p_cap, p_got, w_out, w_cap, w_got: L.fs_digest(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), int(min_words), int(max_gap),
        int(picks), int(cover), int(min_gain), p_out, p_cap, p_got, w_out, w_cap, w_got,
        C.byref(total)), [abi.DIGEST_PICK_DTYPE, abi.DIGEST_WORK_DTYPE], [room, room], "fs_digest")
    return found, works, int(total.value)


def tables(rows, min_words=6, max_gap=0, picks=0, cover=100, min_gain=1, device=0):
    """(picks, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), min_words,
                   max_gap, picks, cover, min_gain, device)


def tables_device(mf, min_words=6, max_gap=0, picks=0, cover=100, min_gain=1, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then says what is wrong)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, n_script, min_words, max_gap, picks,
                   cover, min_gain, device)


def _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, picks, cover, min_gain,
            device):
    if min_words < 1 or min_gain < 1:
        raise ValueError("--min-words and --min-gain must be at least 1")
    if picks < 0:
        raise ValueError("--picks must be at least 0")
    if not 1 <= cover <= 100:
        raise ValueError("--cover must be from 1 to 100")
    found, works, total = find_digest(work, fan, orig, len(names), n_script, min_words, max_gap,
                                      picks, cover, min_gain, device)
    unknown = (UNKNOWN_WORD, '', '')
    n = len(found)
    at = works['subsumed_at'][works['subsumed_at'] != abi.FS_NONE].astype(np.int64)
    like = works['best_pick'][works['best_pick'] != abi.FS_NONE].astype(np.int64)
    subsumed = np.bincount(at, minlength=n + 1)
    represented = np.bincount(like, minlength=n + 1)
    ptab, so_far = [], 0
    for k, p in enumerate(found):
        a, w = int(p['longest_first']), int(p['longest_words'])
        _, char, scene = labels.get(a, unknown)     # (a new run may begin at a bridged word)
        cum = int(p['cum_words'])
        so_far += int(subsumed[k + 1])
        ptab.append([k + 1, names[int(p['work'])], int(p['covered']), int(p['new_words']),
                     int(p['new_runs']), a, a + w - 1, w, char, scene, cum, cum * 100 // total,
                     int(subsumed[k + 1]), so_far, int(represented[k + 1]),
                     ' '.join(labels.get(o, unknown)[0] for o in range(a, a + w))])
    wtab = []
    for v in works:
        covered, inside = int(v['covered']), int(v['in_picks'])
        rank, at, like = int(v['pick_rank']), int(v['subsumed_at']), int(v['best_pick'])
        none = like == abi.FS_NONE
        wtab.append([names[int(v['work'])], covered, '' if rank == abi.FS_NONE else rank, inside,
                     inside * 100 // covered, '' if at == abi.FS_NONE else at,
                     '' if none else like, '' if none else names[int(found[like - 1]['work'])],
                     int(v['best_shared'])])
    return ptab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-digest.csv', '-digest-works.csv'))


def process(args):
    """`ao3.py digest matches [-o PREFIX] [--min-words M] [--max-gap G] [--picks N] [--cover P]
    [--min-gain G] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.picks, args.cover, args.min_gain, args.device)
    return run(args, (PICK_FIELDS, WORK_FIELDS), output_names(args.matches, args.output), tables,
               tables_device, opts)
