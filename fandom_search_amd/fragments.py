"""`ao3.py fragments`: the phrases the fan works quote word for word.

`quotes` merges everything that overlaps into regions and `readings` counts identical spans
only; neither says which exact phrase inside a much-quoted scene everybody quotes.  This command
lists the closed frequent intervals of the script: a stretch [a, b] that WORKS works quote in
full (each in one unbroken run of its coverage) and that loses a work when a word is added on
either side.  A short phrase inside a longer quote is a fragment of its own when more works
quote it, and the nesting shows in the two supports.  A work covers every script word from the
first record of one of its passages to the last, bridged words included; a passage is what
`passages` keeps under the same `--min-words` and `--max-gap`.

Reading, sorting (passages.read_matches / sort_records), ranking and writing are host plumbing;
the passages, the coverage, its runs, the supports and the fragments come from the GPU
(fs_fragments).
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels

FRAGMENT_FIELDS = ['RANK', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'WORDS', 'CHARACTER', 'SCENE',
                   'WORKS', 'EXACT_WORKS', 'LEFT_DROP', 'RIGHT_DROP', 'FIRST_FAN_WORK_FILENAME',
                   'TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'RUNS', 'COVERED_WORDS', 'HELD_FRAGMENTS', 'EXACT_FRAGMENTS',
               'LONGEST_FIRST_WORD_INDEX', 'LONGEST_LAST_WORD_INDEX', 'LONGEST_WORDS',
               'LONGEST_WORKS', 'LONGEST_TEXT']


def find_fragments(work, fan_ix, orig_ix, n_works, n_script, min_words=6, max_gap=0,
                   min_works=2, min_length=3, max_words=128, device=0):
    """(abi.FRAGMENT_DTYPE fragments in (words, first) order, abi.FRAGMENT_WORK_DTYPE per active
    work) of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    n = len(work)
    if not (len(fan) == len(orig) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    return grow(lambda f_out, f_cap, f_got, w_out, w_cap, w_got: L.fs_fragments(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), n, int(n_works), int(n_script), int(min_words), int(max_gap),
        int(min_works), int(min_length), int(max_words), f_out, f_cap, f_got, w_out, w_cap,
        w_got), [abi.FRAGMENT_DTYPE, abi.FRAGMENT_WORK_DTYPE], [4096, 256], "fs_fragments")


def rank_order(frags):
    """The fragments' indices in the order of the CSV: WORKS descending, then WORDS descending,
    then the first word -- one 64-bit key and a stable sort over the (words, first) order the
    library gives."""
    words = frags['last'].astype(np.int64) - frags['first'].astype(np.int64) + 1
    key = (frags['works'].astype(np.int64) << 20) | words      # words <= 4096 < 2^20
    return np.argsort(-key, kind='stable')


def tables(rows, min_words=6, max_gap=0, min_works=2, min_length=3, max_words=128, top=0,
           device=0):
    """(fragments, works): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, _ = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, n_script_of(orig), min_words,
                   max_gap, min_works, min_length, max_words, top, device)


def tables_device(mf, min_words=6, max_gap=0, min_works=2, min_length=3, max_words=128, top=0,
                  device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then says what is wrong)."""
    _, work, fan, orig, _, _ = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, n_script, min_words, max_gap,
                   min_works, min_length, max_words, top, device)


def _tables(labels, names, work, fan, orig, n_script, min_words, max_gap, min_works, min_length,
            max_words, top, device):
    if min_words < 1 or min_works < 1 or min_length < 1:
        raise ValueError("--min-words, --min-works and --min-length must be at least 1")
    if max_words < min_length:
        raise ValueError("--max-words %d is below --min-length %d" % (max_words, min_length))
    if max_words > abi.FS_FRAGMENTS_MAX_WORDS:
        raise ValueError("--max-words %d: at most %d" % (max_words, abi.FS_FRAGMENTS_MAX_WORDS))
    frags, works = find_fragments(work, fan, orig, len(names), n_script, min_words, max_gap,
                                  min_works, min_length, max_words, device)
    unknown = (UNKNOWN_WORD, '', '')

    def text(a, b):
        return ' '.join(labels.get(o, unknown)[0] for o in range(a, b + 1))
    order = rank_order(frags)
    if top:
        order = order[:top]
    ftab = []
    for rank, i in enumerate(order.tolist()):
        f = frags[i]
        a, b = int(f['first']), int(f['last'])
        _, char, scene = labels[a]                  # a fragment starts where a passage starts
        ftab.append([rank + 1, a, b, b - a + 1, char, scene, int(f['works']),
                     int(f['exact_works']), int(f['start_works']), int(f['end_works']),
                     names[int(f['first_work'])], text(a, b)])
    wtab = []
    for v in works:
        a, b, s = int(v['longest_first']), int(v['longest_last']), int(v['longest_works'])
        wtab.append([names[int(v['work'])], int(v['runs']), int(v['covered']), int(v['held']),
                     int(v['exact']), a, b, b - a + 1, '' if s == abi.FS_NONE else s,
                     text(a, b)])
    return ftab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-fragments.csv', '-fragments-works.csv'))


def process(args):
    """`ao3.py fragments matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-works K]
    [--min-length A] [--max-words B] [--top N] [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.min_works, args.min_length, args.max_words,
            args.top, args.device)
    return run(args, (FRAGMENT_FIELDS, WORK_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
