"""`ao3.py variants`: what fans actually wrote at every script word.

A match record pairs FAN_WORK_WORD with ORIGINAL_SCRIPT_WORD, and the two differ: in case and
spelling among strings that share a vector id on the exact path, by real substitutions on the
LSH paths.  This command groups the records by (script word, fan spelling): per pair its
records and the distinct works behind them, the spellings of a script word ranked by records,
then works, then first appearance in the file; and per script word its records, works,
spellings, how many records are verbatim and its top spelling.

The fan words are numbered in first-appearance order: on the device (fs_matches_intern over the
file's bytes, only the first row of every spelling is decoded) or, under the python reader, by
a dict over the rows.  The group-by, the distinct counts and the ranking come from the GPU
(fs_variants); reading labels and writing the CSVs is host plumbing.  Records are taken in file
order: nothing here needs them sorted.
"""

import ctypes as C

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels
from .passages import _FAN_WORD, _FNAME, _ORIG_IX
from .quotes import word_labels

CELL_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_CHARACTER',
               'ORIGINAL_SCRIPT_SCENE', 'RANK', 'FAN_WORK_WORD', 'RECORDS', 'WORKS', 'VERBATIM']
WORD_FIELDS = ['ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'ORIGINAL_SCRIPT_CHARACTER',
               'ORIGINAL_SCRIPT_SCENE', 'RECORDS', 'WORKS', 'SPELLINGS', 'VERBATIM_RECORDS',
               'TOP_FAN_WORD', 'TOP_RECORDS']


def find_variants(work, orig_ix, spell, n_works, n_script, n_spell, device=0):
    """(abi.VARIANT_WORD_DTYPE[n_script], abi.VARIANT_CELL_DTYPE cells in cell order) of records
    in any order."""
    work, orig, spell = abi.as_u32(work), abi.as_u32(orig_ix), abi.as_u32(spell)
    n, n_script = len(work), int(n_script)
    if not (len(orig) == len(spell) == n):
        raise ValueError("columns of different lengths")
    L = _lib.load()
    words = np.zeros(n_script, dtype=abi.VARIANT_WORD_DTYPE)
    cells = grow(lambda out, cap, got: L.fs_variants(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(orig, C.c_uint32),
        abi.ptr(spell, C.c_uint32), n, int(n_works), n_script, int(n_spell),
        words.ctypes.data_as(C.c_void_p), out, cap, got),
        abi.VARIANT_CELL_DTYPE, n, "fs_variants")      # (a cell has a record)
    return words, cells


def fold_key(text, fold_case):
    return text.lower() if fold_case else text


def merge_spellings(texts, fold_case=False):
    """(remap, ids, shown) of spellings listed in first-appearance order: remap[k] = the id of
    texts[k] once equal (and, with fold_case, equal lower-cased) texts are one; ids: key -> id;
    shown[id]: the spelling as its first appearance wrote it."""
    ids, shown = {}, []
    remap = np.empty(len(texts), dtype=np.uint32)
    for k, t in enumerate(texts):
        key = fold_key(t, fold_case)
        j = ids.setdefault(key, len(ids))
        if j == len(shown):
            shown.append(t)
        remap[k] = j
    return remap, ids, shown


def tables(rows, top=10, min_records=1, fold_case=False, device=0):
    """(cells, words): the two CSVs' rows, without headers, for the records `rows`
    (read_matches)."""
    labels = word_labels(rows)
    work_of = {}
    work = np.fromiter((work_of.setdefault(r[_FNAME], len(work_of)) for r in rows),
                       dtype=np.int64, count=len(rows))
    orig = np.fromiter((int(r[_ORIG_IX]) for r in rows), dtype=np.int64, count=len(rows))
    if len(rows) and (orig.min() < 0 or orig.max() >= 1 << 32):
        raise ValueError("word indices outside 0 .. 2^32 - 1")
    spell, ids, shown = merge_spellings([r[_FAN_WORD] for r in rows], fold_case)
    return _tables(labels, ids, shown, work, orig, spell, len(work_of), n_script_of(orig), top,
                   min_records, fold_case, device)


def tables_device(mf, top=10, min_records=1, fold_case=False, device=0):
    """tables over a matches.MatchFile: the fan words numbered on the device, one text decoded
    per spelling and three labels per script word; None when a script word's records spell a
    label in two ways (tables() then decides)."""
    n_script = n_script_of(mf.orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    raw, first = mf.intern(_FAN_WORD)
    remap, ids, shown = merge_spellings(mf.text(_FAN_WORD, first), fold_case)
    spell = np.take(remap, raw) if mf.n else np.zeros(0, dtype=np.uint32)
    return _tables(labels, ids, shown, mf.work, mf.orig, spell, len(mf.names), n_script, top,
                   min_records, fold_case, device)


def _tables(labels, ids, shown, work, orig, spell, n_works, n_script, top, min_records,
            fold_case, device):
    words, cells = find_variants(work, orig, spell, n_works, n_script, len(shown), device)
    have = np.flatnonzero(words['n_records'] > 0)
    # the spelling that is the script word itself, per script word (none: no cell is verbatim)
    same = np.full(n_script, -1, dtype=np.int64)
    for o in have.tolist():
        same[o] = ids.get(fold_key(labels[o][0], fold_case), -1)
    c_orig = cells['orig_ix'].astype(np.int64)
    verbatim = cells['spell'].astype(np.int64) == same[c_orig]
    verbatim_records = np.bincount(c_orig[verbatim], weights=cells['n_records'][verbatim],
                                   minlength=n_script).astype(np.int64)
    first = words['first_cell'].astype(np.int64)
    c_spell, c_rec = cells['spell'].tolist(), cells['n_records'].tolist()
    c_works, c_verb = cells['n_works'].tolist(), verbatim.tolist()
    ctab, wtab = [], []
    for o in have.tolist():
        word, char, scene = labels[o]
        w, a = words[o], int(first[o])
        wtab.append([o, word, char, scene, int(w['n_records']), int(w['n_works']),
                     int(w['n_spellings']), int(verbatim_records[o]), shown[c_spell[a]],
                     c_rec[a]])
        keep = int(w['n_spellings'])
        if top:
            keep = min(keep, top)
        for k in range(keep):
            c = a + k
            if c_rec[c] < min_records:
                continue
            ctab.append([o, word, char, scene, k + 1, shown[c_spell[c]], c_rec[c], c_works[c],
                         1 if c_verb[c] else 0])
    return ctab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix, ('-variants.csv', '-variants-words.csv'))


def process(args):
    """`ao3.py variants matches [-o PREFIX] [--top K] [--min-records R] [--fold-case]
    [--device D] [--reader {device,python}]`."""
    opts = (args.top, args.min_records, args.fold_case, args.device)
    return run(args, (CELL_FIELDS, WORD_FIELDS), output_names(args.matches, args.output),
               tables, tables_device, opts)
