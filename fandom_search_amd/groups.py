"""`ao3.py groups`: the reuse of a match CSV by groups of fan works, the groups taken from the
metadata CSV `getmeta` writes (one row per work: FILENAME, TITLE, AUTHOR, SUMMARY, NOTES,
PUBLICATION_DATE, LANGUAGE, TAGS).

`works` reduces the records by work and `quotes` by script word over all works.  This command
answers which lines the works of one year, one author, one language or one tag quote: per
group its works, records and passages, the script words its works cover and how many of them
cover each (the depth), the group x scene matrix and the (group, script word) rows of depth >=
`--min-works`.  A work can be in many groups (a tag is one group among its work's twenty), and
the figures are distinct counts, so they are not sums of the per-work rows.

Reading the two files, the keys and the join by file stem are host plumbing; the passages, the
coverage and the reduction by group come from the GPU (fs_groups).  A passage is what
`passages` keeps under the same `--min-words` and `--max-gap`, and the coverage of a work is
that of `pairs`.
"""

import csv
import ctypes as C
import json
import os
import re

import numpy as np

from . import _lib, abi
from .command import grow, n_script_of, prefixed, run, script_labels, work_names
from .passages import sort_records
from .quotes import UNKNOWN_WORD, word_labels
from .works import groups_of_labels

META_FIELDS = ['FILENAME', 'TITLE', 'AUTHOR', 'SUMMARY', 'NOTES', 'PUBLICATION_DATE', 'LANGUAGE',
               'TAGS']
GROUP_FIELDS = ['GROUP', 'WORKS_IN_META', 'WORKS_WITH_RECORDS', 'WORKS_WITH_PASSAGES',
                'MATCHED_WORDS', 'EXACT_WORDS', 'PASSAGES', 'WORDS_IN_PASSAGES',
                'LONGEST_PASSAGE', 'COVERED_WORDS', 'PEAK_DEPTH', 'PEAK_WORD_INDEX', 'TOP_SCENE',
                'TOP_SCENE_WORDS']
SCENE_FIELDS = ['GROUP', 'SCENE', 'MATCHED_WORDS', 'EXACT_WORDS', 'WORKS']
WORD_FIELDS = ['GROUP', 'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'CHARACTER',
               'SCENE', 'WORKS']
NO_VALUE, UNKNOWN_DATE, NO_METADATA, EMPTY = '(none)', '(unknown date)', '(no metadata)', '(empty)'
LAST_GROUPS = (NO_VALUE, UNKNOWN_DATE, NO_METADATA)       # after every other key, in this order
BY = ('year', 'month', 'author', 'language', 'tag')
_COLUMN = {'year': 'PUBLICATION_DATE', 'month': 'PUBLICATION_DATE', 'author': 'AUTHOR',
           'language': 'LANGUAGE', 'tag': 'TAGS'}
_DATE = re.compile(r'\d{4}-\d{2}-\d{2}')


def check_by(by):
    """`by` split into (kind, tag category or None); ValueError for an unknown one."""
    if by in BY:
        return by, None
    if by.startswith('tag:') and len(by) > 4:
        return 'tag', by[4:]
    raise ValueError("--by takes year, month, author, language, tag or tag:<Category>, not %r" % by)


def stem(name):
    """The base name without its last extension: what joins a work to its metadata row."""
    return os.path.splitext(os.path.basename(name))[0]


def read_meta(path, by='year'):
    """{stem: row} of the metadata CSV; ValueError for a file without FILENAME or without the
    column `by` needs, and for two rows of one stem."""
    kind, _ = check_by(by)
    meta = {}
    with open(path, newline='', encoding='utf-8') as fh:
        reader = csv.DictReader(fh)
        fields = reader.fieldnames or []
        for col in ('FILENAME', _COLUMN[kind]):
            if col not in fields:
                raise ValueError("%s has no %s column" % (path, col))
        for row in reader:
            s = stem(row['FILENAME'] or '')
            if s in meta:
                raise ValueError("%s has two rows for the work %r" % (path, s))
            meta[s] = row
    return meta


def _tags(row):
    try:
        tags = json.loads(row['TAGS'] or '')
    except ValueError:
        tags = None
    if not isinstance(tags, dict) or not all(isinstance(v, str) for v in tags.values()):
        raise ValueError("the TAGS of %r are not a JSON object of strings" % row['FILENAME'])
    return tags


def keys_of(row, by):
    """The group keys of one metadata row under `by`, in a fixed order, never empty."""
    kind, category = check_by(by)
    if kind in ('year', 'month'):
        date = (row['PUBLICATION_DATE'] or '').strip()
        return [date[:4 if kind == 'year' else 7]] if _DATE.fullmatch(date) else [UNKNOWN_DATE]
    if kind != 'tag':
        return [(row[_COLUMN[kind]] or '').strip() or EMPTY]
    keys = []
    for cat, value in _tags(row).items():
        if category is not None and cat != category:
            continue
        for v in value.split('; '):
            v = v.strip()
            if v:
                keys.append(v if category is not None else '%s: %s' % (cat, v))
    return list(dict.fromkeys(keys)) or [NO_VALUE]


def membership(names, meta, by='year'):
    """(group keys in group order, mem_off[len(names) + 1], mem_grp, metadata rows per group)
    for the works `names` of a match file and read_meta's rows: work w is in the groups
    mem_grp[mem_off[w]:mem_off[w + 1]], ascending."""
    seen = {}
    for name in names:
        if seen.setdefault(stem(name), name) != name:
            raise ValueError("the works %r and %r of the match file are one work, %r"
                             % (seen[stem(name)], name, stem(name)))
    keys_at = {s: keys_of(row, by) for s, row in meta.items()}
    in_meta = {}
    for keys in keys_at.values():
        for k in keys:
            in_meta[k] = in_meta.get(k, 0) + 1
    of_work = [keys_at.get(stem(name), [NO_METADATA]) for name in names]
    found = set(in_meta).union(*of_work) if of_work else set(in_meta)
    labels = (sorted(k for k in found if k not in LAST_GROUPS) +
              [k for k in LAST_GROUPS if k in found])
    number = {k: g for g, k in enumerate(labels)}
    mem_off = np.zeros(len(names) + 1, dtype=np.uint64)
    mem_grp = []
    for w, keys in enumerate(of_work):
        mem_grp += sorted(number[k] for k in keys)
        mem_off[w + 1] = len(mem_grp)
    return (labels, mem_off, np.array(mem_grp, dtype=np.uint32),
            [in_meta.get(k, 0) for k in labels])


def find_groups(work, fan_ix, orig_ix, exact, n_works, n_script, mem_off, mem_grp, n_groups,
                label_of=None, n_labels=0, min_words=6, max_gap=0, min_works=1, device=0):
    """(abi.GROUP_DTYPE[n_groups], abi.GROUP_CELL_DTYPE cells in (group, label) order,
    abi.GROUP_WORD_DTYPE rows in (group, word) order) of records sorted by (work, fan_ix)."""
    work, fan, orig = abi.as_u32(work), abi.as_u32(fan_ix), abi.as_u32(orig_ix)
    exact = np.ascontiguousarray(exact, dtype=np.uint8)
    mem_off, mem_grp = abi.as_u64(mem_off), abi.as_u32(mem_grp)
    n, n_works, n_groups, n_labels = len(work), int(n_works), int(n_groups), int(n_labels)
    if not (len(fan) == len(orig) == len(exact) == n):
        raise ValueError("columns of different lengths")
    if len(mem_off) != n_works + 1:
        raise ValueError("mem_off needs one entry per work and one more")
    lab = None
    if n_labels:
        lab = abi.as_u32(label_of)
        if len(lab) != int(n_script):
            raise ValueError("label_of needs one entry per script word")
    L = _lib.load()
    groups = np.zeros(n_groups, dtype=abi.GROUP_DTYPE)
    cells, words = grow(lambda *outs: L.fs_groups(
        int(device), abi.ptr(work, C.c_uint32), abi.ptr(fan, C.c_uint32),
        abi.ptr(orig, C.c_uint32), abi.ptr(exact, C.c_uint8), n, n_works, int(n_script),
        abi.ptr(mem_off, C.c_uint64), abi.ptr(mem_grp, C.c_uint32), n_groups,
        abi.ptr(lab, C.c_uint32), n_labels, int(min_words), int(max_gap), int(min_works),
        groups.ctypes.data_as(C.c_void_p), *outs),
        [abi.GROUP_CELL_DTYPE, abi.GROUP_WORD_DTYPE], [4096, 1 << 16], "fs_groups")
    return groups, cells, words


def tables(rows, meta, by='year', min_words=6, max_gap=0, min_works=1, device=0):
    """(groups, scenes, words): the three CSVs' rows, without headers, for the records `rows`
    (read_matches) and the metadata rows `meta` (read_meta)."""
    labels = word_labels(rows)
    _, work, fan, orig, _, comb = sort_records(rows)
    return _tables(labels, work_names(rows), work, fan, orig, comb, n_script_of(orig), meta, by,
                   min_words, max_gap, min_works, device)


def tables_device(mf, meta, by='year', min_words=6, max_gap=0, min_works=1, device=0):
    """tables over a matches.MatchFile, the three labels decoded once per script word; None
    when a script word's records spell one in two ways (tables() then decides)."""
    _, work, fan, orig, _, comb = mf.sorted()
    n_script = n_script_of(orig)
    labels = script_labels(mf, n_script)
    if labels is None:
        return None
    return _tables(labels, list(mf.names), work, fan, orig, comb, n_script, meta, by, min_words,
                   max_gap, min_works, device)


def _tables(labels, names, work, fan, orig, comb, n_script, meta, by, min_words, max_gap,
            min_works, device):
    keys, mem_off, mem_grp, in_meta = membership(names, meta, by)
    scene_of, scenes = groups_of_labels({o: lab[2] for o, lab in labels.items()}, n_script)
    exact = np.asarray(comb, dtype=np.float64) <= 0
    groups, cells, words = find_groups(work, fan, orig, exact, len(names), n_script, mem_off,
                                       mem_grp, len(keys), scene_of, len(scenes), min_words,
                                       max_gap, min_works, device)
    gtab = []
    for g, key in enumerate(keys):
        v = groups[g]
        first, top = int(v['peak_first']), int(v['top_label'])
        gtab.append([key, in_meta[g], int(v['n_works']), int(v['n_passage_works']),
                     int(v['n_words']), int(v['n_exact']), int(v['n_passages']),
                     int(v['passage_words']), int(v['longest']), int(v['covered']),
                     int(v['peak']), '' if first == abi.FS_NONE else first,
                     '' if top == abi.FS_NONE else scenes[top], int(v['top_label_words'])])
    stab = [[keys[int(c['group'])], scenes[int(c['label'])], int(c['n_words']),
             int(c['n_exact']), int(c['n_works'])] for c in cells]
    unknown = (UNKNOWN_WORD, '', '')
    wtab = []
    for r in words:
        o = int(r['orig_ix'])
        word, char, scene = labels.get(o, unknown)
        wtab.append([keys[int(r['group'])], o, word, char, scene, int(r['n_works'])])
    return gtab, stab, wtab


def output_names(matches, prefix=None):
    return prefixed(matches, prefix,
                    ('-groups.csv', '-groups-scenes.csv', '-groups-words.csv'))


def process(args):
    """`ao3.py groups matches meta [--by B] [-o PREFIX] [--min-words M] [--max-gap G]
    [--min-works K] [--device D] [--reader {device,python}]`."""
    meta = read_meta(args.meta, args.by)            # (small: always read on the host)
    for row in meta.values():
        keys_of(row, args.by)                       # (a malformed row stops before the GPU)
    opts = (meta, args.by, args.min_words, args.max_gap, args.min_works, args.device)
    return run(args, (GROUP_FIELDS, SCENE_FIELDS, WORD_FIELDS),
               output_names(args.matches, args.output), tables, tables_device, opts)
