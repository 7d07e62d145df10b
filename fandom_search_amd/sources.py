"""`ao3.py sources`: which script is each fan passage quoting?

`search` takes several scripts and leaves one match CSV per script; every other command reads
one of them.  This one joins them.  The passages of each file (what `passages` keeps under the
same `--min-words` and `--max-gap`) are laid on the fan works' words: two passages of different
scripts in one work whose fan spans share a word are rivals.  A passage without a rival is
`alone`; one whose key (matched words, exact words, then the earlier script) beats every
rival's has `won`; every other has `lost` -- a local maximum on purpose, so a passage that
loses to a passage which itself lost is still `lost`.  Per passage: its rivals, the scripts
among them, the words of its span a rival also covers (a union) and the words it holds alone,
and its best rival.  Per (work, script), per script and per pair of scripts: the sums.

Works are one work across files when their FAN_WORK_FILENAME is equal and are numbered by
first appearance through the files in argument order.  Reading, numbering, the stable (work,
FAN_WORK_WORD_INDEX) order of each file and writing are host plumbing; the passages, the
interval join and every figure come from the GPU (fs_sources).
"""

import ctypes as C
import os

import numpy as np

from . import _lib, abi
from .command import grow, prefixed, work_names, write_tables
from .passages import _CHAR, _FAN_WORD, _ORIG_WORD, _SCENE, read_matches, sort_records

PASSAGE_FIELDS = ['SCRIPT', 'FAN_WORK_FILENAME', 'FAN_WORK_WORD_START', 'FAN_WORK_WORD_END',
                  'ORIGINAL_SCRIPT_WORD_START', 'ORIGINAL_SCRIPT_WORD_END', 'MATCHED_WORDS',
                  'EXACT_WORDS', 'ORIGINAL_SCRIPT_CHARACTER', 'ORIGINAL_SCRIPT_SCENE', 'RIVALS',
                  'RIVAL_SCRIPTS', 'CONTESTED_WORDS', 'SOLE_WORDS', 'OUTCOME', 'BEST_RIVAL',
                  'BEST_RIVAL_WORDS', 'BEST_RIVAL_FAN_START', 'FAN_WORK_TEXT',
                  'ORIGINAL_SCRIPT_TEXT']
WORK_FIELDS = ['FAN_WORK_FILENAME', 'SCRIPT', 'PASSAGES', 'ALONE', 'WON', 'LOST', 'COVERED_WORDS',
               'CONTESTED_WORDS', 'SOLE_WORDS', 'WORK_SCRIPTS', 'PRIMARY']
SCRIPT_FIELDS = ['SCRIPT', 'WORKS', 'PASSAGES', 'ALONE', 'WON', 'LOST', 'COVERED_WORDS',
                 'CONTESTED_WORDS', 'SOLE_WORDS', 'PRIMARY_WORKS']
PAIR_FIELDS = ['SCRIPT_A', 'SCRIPT_B', 'WORKS_BOTH', 'CONTESTS', 'SHARED_WORDS', 'A_WINS',
               'B_WINS']
OUTCOMES = ('alone', 'won', 'lost')      # abi.FS_SOURCE_ALONE, _WON, _LOST
SUFFIXES = ('-sources.csv', '-sources-works.csv', '-sources-scripts.csv', '-sources-pairs.csv')


def find_sources(files, n_works, min_words=6, max_gap=0, device=0):
    """(abi.SOURCE_PASSAGE_DTYPE passages in (work, fan_first, script, first) order,
    abi.SOURCE_WORK_DTYPE rows in (work, script) order, abi.SOURCE_SCRIPT_DTYPE[K],
    abi.SOURCE_PAIR_DTYPE[K (K - 1) / 2]) of K files, each (work, fan_ix, orig_ix, comb) sorted
    by (work, fan_ix) with the work numbers shared by all files."""
    K = len(files)
    keep, cols = [], (abi.FsSourceCols * max(1, K))()
    for s, (work, fan, orig, comb) in enumerate(files):
        work, fan, orig = abi.as_u32(work), abi.as_u32(fan), abi.as_u32(orig)
        comb = np.ascontiguousarray(comb, dtype=np.float64)
        if not (len(fan) == len(orig) == len(comb) == len(work)):
            raise ValueError("columns of different lengths")
        keep.append((work, fan, orig, comb))
        cols[s] = abi.FsSourceCols(abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
                                   abi.ptr(orig, C.c_uint32), abi.ptr(comb, C.c_double),
                                   len(work))
    L = _lib.load()
    scripts = np.zeros(K, dtype=abi.SOURCE_SCRIPT_DTYPE)
    pairs = np.zeros(K * (K - 1) // 2, dtype=abi.SOURCE_PAIR_DTYPE)
    passages, works = grow(lambda *outs: L.fs_sources(
        int(device), cols, K, int(n_works), int(min_words), int(max_gap), *outs,
        scripts.ctypes.data_as(C.c_void_p), pairs.ctypes.data_as(C.c_void_p)),
        [abi.SOURCE_PASSAGE_DTYPE, abi.SOURCE_WORK_DTYPE], [4096, 4096], "fs_sources")
    return passages, works, scripts, pairs


def script_names(paths, names=None):
    """The scripts' names: `names` (a list, or 'A,B,...'); else the files' parent directories
    when these differ pairwise (the layout a several-script `search` writes); else the file
    names without .csv.  ValueError for fewer than two files, a `names` of another length or
    names that are still equal."""
    paths = list(paths)
    if len(paths) < 2:
        raise ValueError("sources joins the match files of at least two scripts, not %d"
                         % len(paths))
    if names is not None:
        got = names.split(',') if isinstance(names, str) else list(names)
        if len(got) != len(paths):
            raise ValueError("--names has %d names for %d files" % (len(got), len(paths)))
    else:
        got = [os.path.basename(os.path.dirname(os.path.abspath(p))) for p in paths]
        if len(set(got)) != len(got):
            got = [os.path.basename(p) for p in paths]
            got = [g[:-4] if g.endswith('.csv') else g for g in got]
    if len(set(got)) != len(got):
        raise ValueError("two scripts are both named %r: give --names"
                         % sorted(g for g in got if got.count(g) > 1)[0])
    return got


class _PythonFile:
    """A match file through read_matches: `names` (its works by first appearance), sorted()
    as sort_records, text(column, records)."""

    def __init__(self, path):
        self.rows = read_matches(path)
        self.names = work_names(self.rows)

    def sorted(self):
        return sort_records(self.rows)

    def text(self, column, records):
        return [self.rows[i][column] for i in np.asarray(records).tolist()]


def open_file(path, reader, device=0):
    """The match file `path` under `reader`: a matches.MatchFile, or, under 'python' or for a
    file the device reader does not take, a _PythonFile."""
    if reader == 'device':
        from .matches import MatchFile
        mf = MatchFile(path, device)
        if not mf.outside:
            return mf
        mf.close()
    return _PythonFile(path)


def shared_order(files):
    """(work names, per file (order, work, fan, orig, comb)): the works numbered by first
    appearance through the files in turn, every file in stable (work, fan_ix) order."""
    number, out = {}, []
    for f in files:
        to_global = np.fromiter((number.setdefault(n, len(number)) for n in f.names),
                                dtype=np.int64, count=len(f.names))
        order, work, fan, orig, _, comb = f.sorted()
        work = to_global[work] if len(work) else np.zeros(0, dtype=np.int64)
        if len(to_global) > 1 and not bool(np.all(to_global[1:] > to_global[:-1])):
            again = np.lexsort((fan, work))             # stable: ties keep the file's order
            order, work, fan, orig, comb = (order[again], work[again], fan[again], orig[again],
                                            comb[again])
        out.append((order, work, fan, orig, comb))
    return list(number), out


def tables(files, names, min_words=6, max_gap=0, device=0, find=find_sources):
    """The four CSVs' rows, without headers, of the opened match files `files` (open_file) and
    their scripts' names."""
    work_names, cols = shared_order(files)
    found = find([c[1:] for c in cols], len(work_names), min_words, max_gap, device)
    return _rows_of(found, files, [c[0] for c in cols], names, work_names)


def _texts(f, order, first, count):
    """Per passage (fan text, script text, character, scene) of file f, decoding only the
    records inside the passages."""
    first, count = first.astype(np.int64), count.astype(np.int64)
    ends = np.cumsum(count)
    pos = np.repeat(first - (ends - count), count) + np.arange(ends[-1] if len(ends) else 0)
    recs = order[pos]
    fan_words, orig_words = f.text(_FAN_WORD, recs), f.text(_ORIG_WORD, recs)
    heads = order[first]
    chars, scenes = f.text(_CHAR, heads), f.text(_SCENE, heads)
    return [(' '.join(fan_words[int(e - k):int(e)]), ' '.join(orig_words[int(e - k):int(e)]),
             chars[j], scenes[j]) for j, (e, k) in enumerate(zip(ends, count))]


def _rows_of(found, files, orders, names, work_names):
    passages, works, scripts, pairs = found
    text_of = {}
    for s, f in enumerate(files):
        mine = np.flatnonzero(passages['script'] == s)
        got = _texts(f, orders[s], passages['first'][mine], passages['n_words'][mine])
        text_of.update(zip(mine.tolist(), got))
    ptab = []
    for j, p in enumerate(passages):
        fan_text, orig_text, char, scene = text_of[j]
        alone = int(p['outcome']) == abi.FS_SOURCE_ALONE
        ptab.append([names[int(p['script'])], work_names[int(p['work'])], int(p['fan_first']),
                     int(p['fan_last']), int(p['orig_first']), int(p['orig_last']),
                     int(p['n_words']), int(p['n_exact']), char, scene, int(p['rivals']),
                     int(p['rival_scripts']), int(p['contested_words']), int(p['sole_words']),
                     OUTCOMES[int(p['outcome'])],
                     '' if alone else names[int(p['best_rival'])],
                     '' if alone else int(p['best_rival_words']),
                     '' if alone else int(p['best_rival_fan_first']), fan_text, orig_text])
    wtab = [[work_names[int(r['work'])], names[int(r['script'])]]
            + [int(r[k]) for k in ('passages', 'alone', 'won', 'lost', 'covered_words',
                                   'contested_words', 'sole_words', 'work_scripts', 'primary')]
            for r in works]
    stab = [[names[s]] + [int(r[k]) for k in ('works', 'passages', 'alone', 'won', 'lost',
                                               'covered_words', 'contested_words', 'sole_words',
                                               'primary_works')]
            for s, r in enumerate(scripts)]
    qtab = [[names[int(r['a'])], names[int(r['b'])]]
            + [int(r[k]) for k in ('works_both', 'contests', 'shared_words', 'a_wins', 'b_wins')]
            for r in pairs]
    return ptab, wtab, stab, qtab


def output_names(prefix):
    return prefixed(None, prefix, SUFFIXES)


def process(args):
    """`ao3.py sources matches matches [...] -o PREFIX [--names A,B,...] [--min-words M]
    [--max-gap G] [--device D] [--reader {device,python}]`."""
    from .matches import reader_of
    names = script_names(args.matches, args.names)
    reader = reader_of(args)
    files = [open_file(p, reader, args.device) for p in args.matches]
    try:
        body = tables(files, names, args.min_words, args.max_gap, args.device)
    finally:
        for f in files:
            if hasattr(f, 'close'):
                f.close()
    outs = output_names(args.output)
    write_tables(outs, (PASSAGE_FIELDS, WORK_FIELDS, SCRIPT_FIELDS, PAIR_FIELDS), body)
    return outs
