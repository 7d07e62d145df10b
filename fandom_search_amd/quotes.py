"""`ao3.py quotes`: the per-word match records of a search seen from the script's side.

`format` counts records per script word, `passages` lists every reused span of every fan work,
`works` reduces the records by fan work.  This command answers which stretches of the script
fans quote and how many different works quote each one: per script word the distinct works
behind its records and behind the passages covering it (its depth), and the regions, maximal
stretches of depth >= `--min-works`, ranked material for a reader: their passages, works,
matched words and the peak of the depth with where it lies.

Reading, sorting (passages.read_matches / sort_records) and writing are host plumbing; the
passages, the distinct counts and the regions come from the GPU (fs_quotes).  A passage is what
`passages` keeps under the same `--min-words` and `--max-gap`; it covers every script word
between its first and last record, bridged ones included.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import _CHAR, _ORIG_IX, _ORIG_WORD, _SCENE, sort_records

REGION_FIELDS = ['ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'WORDS',
                 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'PASSAGES', 'WORKS',
                 'MATCHED_WORDS', 'EXACT_WORDS', 'PEAK_WORKS', 'PEAK_WORD_START',
                 'PEAK_WORD_END', 'ORIGINAL_SCRIPT_TEXT']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'MATCHED_WORDS',
               'EXACT_WORDS', 'WORKS', 'PASSAGES', 'PASSAGE_WORKS', 'REGION']
UNKNOWN_WORD = '[?]'       # a bridged script word no record names (no single token looks so)


def find_quotes(work, fan_ix, orig_ix, comb, n_works, n_script, min_words=6, max_gap=0,
                min_works=1, device=0):
    """(abi.QUOTE_WORD_DTYPE[n_script], abi.QUOTE_REGION_DTYPE regions in script order) of
    records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    comb = np.ascontiguousarray(comb, dtype=np.float64)
    n, n_script = len(work), int(n_script)
    if not (len(fan) == len(orig) == len(comb) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    words = np.zeros(n_script, dtype=abi.QUOTE_WORD_DTYPE)
    cap = min(n, (n_script + 1) // 2, 4096)         # regions lie a word apart at least
    regions = grow(lambda out, cap, got: L.fs_quotes(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(comb, C.c_double), n, int(n_works), n_script,
        int(min_words), int(max_gap), int(min_works), words.ctypes.data_as(C.c_void_p), out,
        cap, got), abi.QUOTE_REGION_DTYPE, cap, "fs_quotes")
    return words, regions


def word_labels(rows):
    """{script word index: (word, character, scene)} of the records `rows`; ValueError for a
    script word that carries two different texts, characters or scenes."""
    labels = {}
    for r in rows:
        o = int(r[_ORIG_IX])
        lab = (r[_ORIG_WORD], r[_CHAR], r[_SCENE])
        have = labels.setdefault(o, lab)
        if have != lab:
            what, a, b = next((w, x, y) for w, x, y in zip(('word', 'character', 'scene'), have, lab)
                              if x != y)
            raise ValueError("script word %d has two %ss, %r and %r: records of different "
                             "scripts in one file?" % (o, what, a, b))
    return labels


def tables(rows, min_words=6, max_gap=0, min_works=1, device=0):
    """(regions, words): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work, fan, orig, comb, len(work_names(rows)), n_script_of(orig),
                   min_words, max_gap, min_works, device)


def tables_device(mf, min_words=6, max_gap=0, min_works=1, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, work, fan, orig, comb, len(mf.names), n_script, min_words, max_gap,
                   min_works, device)


def _tables(labels, work, fan, orig, comb, n_works, n_script, min_words, max_gap, min_works,
            device):
    words, regions = find_quotes(work, fan, orig, comb, n_works, n_script, min_words, max_gap,
                                 min_works, device)
    unknown = (UNKNOWN_WORD, '', '')
    rtab = []
    for r in regions:
        a, b = int(r['first']), int(r['last'])
        _, char, scene = labels[a]                  # a region starts at a record
        rtab.append([a, b, b - a + 1, char, scene, int(r['n_passages']), int(r['n_works']),
                     int(r['n_words']), int(r['n_exact']), int(r['peak']), int(r['peak_first']),
                     int(r['peak_last']),
                     ' '.join(labels.get(o, unknown)[0] for o in range(a, b + 1))])
    wtab = []
    for o in np.nonzero((words['n_words'] > 0) | (words['n_passages'] > 0))[0].tolist():
        w = words[o]
        region = int(w['region'])
        wtab.append([o, labels.get(o, unknown)[0], int(w['n_words']), int(w['n_exact']),
                     int(w['n_works']), int(w['n_passages']), int(w['n_passage_works']),
                     '' if region == abi.FS_NONE else region + 1])
    return rtab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-quotes.csv', '-quotes-words.csv'))


def process(args):
    """`ao3.py quotes matches [-o PREFIX] [--min-words M] [--max-gap G] [--min-works K]
    [--device D] [--reader {device,python}]`."""
    opts = (args.min_words, args.max_gap, args.min_works, args.device)
    return run(args, (REGION_FIELDS, WORD_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
