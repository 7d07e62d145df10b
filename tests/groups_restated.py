"""The `groups` contract restated in plain Python, a set of script words per work and a loop
per group: the oracle of the tests (tests/test_groups_host.py, tests/test_gpu_groups.py) and of
the committed tests/golden/groups_*.csv.  The product never imports it.  The passage rule is
that of tests/quotes_restated.py and the coverage that of tests/pairs_restated.py."""

import csv
import io
import json
import os
import re

from tests import pairs_restated as pp
from tests import passages_restated as pr

NONE = 0xFFFFFFFF
GROUP_FIELDS = ['GROUP', 'WORKS_IN_META', 'WORKS_WITH_RECORDS', 'WORKS_WITH_PASSAGES',
                'MATCHED_WORDS', 'EXACT_WORDS', 'PASSAGES', 'WORDS_IN_PASSAGES',
                'LONGEST_PASSAGE', 'COVERED_WORDS', 'PEAK_DEPTH', 'PEAK_WORD_INDEX', 'TOP_SCENE',
                'TOP_SCENE_WORDS']
SCENE_FIELDS = ['GROUP', 'SCENE', 'MATCHED_WORDS', 'EXACT_WORDS', 'WORKS']
WORD_FIELDS = ['GROUP', 'ORIGINAL_SCRIPT_WORD_INDEX', 'ORIGINAL_SCRIPT_WORD', 'CHARACTER',
               'SCENE', 'WORKS']
GROUP_KEYS = ['n_works', 'n_passage_works', 'n_words', 'n_exact', 'n_passages', 'passage_words',
              'longest', 'covered', 'peak', 'peak_first', 'top_label', 'top_label_words',
              'n_cells', 'n_word_rows']
CELL_KEYS = ['group', 'label', 'n_words', 'n_exact', 'n_works']
WORD_KEYS = ['group', 'orig_ix', 'n_works']
UNKNOWN_WORD = '[?]'
LAST = ['(none)', '(unknown date)', '(no metadata)']


def groups(records, n_works, n_script, members_of, n_groups, label_of=None, n_labels=0,
           min_words=6, max_gap=0, min_works=1):
    """records: (work, fan_ix, orig_ix, exact) tuples sorted by (work, fan_ix); members_of[w]:
    the groups of work w, strictly ascending.  Returns (one dict of GROUP_KEYS per group, cells
    as dicts of CELL_KEYS in (group, label) order, word rows as dicts of WORD_KEYS in (group,
    word) order)."""
    if min_words < 1 or min_works < 1:
        raise ValueError("min_words and min_works must be at least 1")
    if len(members_of) != n_works:
        raise ValueError("one membership list per work")
    for gs in members_of:
        if any(g >= n_groups for g in gs) or any(a >= b for a, b in zip(gs, gs[1:])):
            raise ValueError("membership outside the groups or not strictly ascending")
    if n_labels and (len(label_of) != n_script or any(l >= n_labels for l in label_of)):
        raise ValueError("label_of outside the labels")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = pp.coverage(records, n_works, min_words, max_gap)      # (raises on unsorted records)
    lengths = [[] for _ in range(n_works)]
    for p in pr.passages([tuple(r[:3]) + (0.0, 0.0) for r in records], min_words, max_gap):
        lengths[records[p['first']][0]].append(p['n_words'])
    of_work = [[] for _ in range(n_works)]
    for r in records:
        of_work[r[0]].append(r)
    out, cells, rows = [], [], []
    for g in range(n_groups):
        works = [w for w in range(n_works) if g in members_of[w]]
        recs = [r for w in works for r in of_work[w]]
        spans = [n for w in works for n in lengths[w]]
        depth = [sum(1 for w in works if o in cov[w]) for o in range(n_script)]
        peak = max(depth, default=0)
        d = dict(n_works=sum(1 for w in works if of_work[w]),
                 n_passage_works=sum(1 for w in works if lengths[w]),
                 n_words=len(recs), n_exact=sum(1 for r in recs if r[3]),
                 n_passages=len(spans), passage_words=sum(spans), longest=max(spans, default=0),
                 covered=sum(1 for x in depth if x), peak=peak,
                 peak_first=depth.index(peak) if peak else NONE,
                 top_label=NONE, top_label_words=0, n_cells=0, n_word_rows=0)
        if n_labels:
            mine = []
            for lab in range(n_labels):
                at = [r for r in recs if label_of[r[2]] == lab]
                if at:
                    mine.append(dict(group=g, label=lab, n_words=len(at),
                                     n_exact=sum(1 for r in at if r[3]),
                                     n_works=len(set(r[0] for r in at))))
            if mine:
                top = max(mine, key=lambda c: (c['n_words'], -c['label']))
                d.update(top_label=top['label'], top_label_words=top['n_words'])
            d['n_cells'] = len(mine)
            cells += mine
        mine = [dict(group=g, orig_ix=o, n_works=x) for o, x in enumerate(depth)
                if x >= min_works]
        d['n_word_rows'] = len(mine)
        rows += mine
        out.append(d)
    return out, cells, rows


# ---- the metadata file -------------------------------------------------------------------

def stem(name):
    base = os.path.basename(name)
    dot = base.rfind('.')
    return base[:dot] if dot > 0 else base


def keys_of(row, by):
    if by in ('year', 'month'):
        date = row['PUBLICATION_DATE'].strip()
        if not re.fullmatch(r'[0-9]{4}-[0-9]{2}-[0-9]{2}', date):
            return ['(unknown date)']
        return [date[:4]] if by == 'year' else [date[:7]]
    if by in ('author', 'language'):
        return [row[by.upper()].strip() or '(empty)']
    if by != 'tag' and not (by.startswith('tag:') and by[4:]):
        raise ValueError("unknown --by %r" % by)
    try:
        tags = json.loads(row['TAGS'])
    except ValueError:
        tags = None
    if not isinstance(tags, dict) or any(not isinstance(v, str) for v in tags.values()):
        raise ValueError("the TAGS of %r are not a JSON object of strings" % row['FILENAME'])
    only = by[4:] if by != 'tag' else None
    keys = []
    for cat, text in tags.items():
        if only is not None and cat != only:
            continue
        for part in text.split('; '):
            part = part.strip()
            key = part if only is not None else cat + ': ' + part
            if part and key not in keys:
                keys.append(key)
    return keys or ['(none)']


def read_meta(text, by):
    """{stem: row} of a metadata CSV's text."""
    reader = csv.DictReader(io.StringIO(text, newline=''))
    need = {'year': 'PUBLICATION_DATE', 'month': 'PUBLICATION_DATE', 'author': 'AUTHOR',
            'language': 'LANGUAGE'}.get(by, 'TAGS')
    if 'FILENAME' not in (reader.fieldnames or []) or need not in reader.fieldnames:
        raise ValueError("the metadata has no FILENAME or no %s column" % need)
    meta = {}
    for row in reader:
        if stem(row['FILENAME']) in meta:
            raise ValueError("two metadata rows for %r" % stem(row['FILENAME']))
        meta[stem(row['FILENAME'])] = row
    return meta


def membership(names, meta, by):
    """(group keys in order, the groups of every work, metadata rows per group)."""
    stems = [stem(n) for n in names]
    for s in stems:
        if stems.count(s) > 1:
            raise ValueError("two works of the match file are %r" % s)
    rows_with = {}
    for row in meta.values():
        for k in keys_of(row, by):
            rows_with[k] = rows_with.get(k, 0) + 1
    per_work = [keys_of(meta[s], by) if s in meta else ['(no metadata)'] for s in stems]
    every = set(rows_with)
    for keys in per_work:
        every.update(keys)
    order = sorted(k for k in every if k not in LAST) + [k for k in LAST if k in every]
    members_of = [sorted(order.index(k) for k in keys) for keys in per_work]
    return order, members_of, [rows_with.get(k, 0) for k in order]


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def groups_csv(text, meta_text, by='year', min_words=6, max_gap=0, min_works=1):
    """The bytes `ao3.py groups` writes for a match CSV's text and a metadata CSV's text:
    (groups, groups-scenes, groups-words)."""
    meta = read_meta(meta_text, by)
    for row in meta.values():
        keys_of(row, by)
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4]), pr._num(rows[k][11]) <= 0) for w, f, k in keyed]
    names = list(work_of)
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        if label.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
    n_script = max(label) + 1 if label else 0
    scenes = []
    label_of = [0] * n_script                         # (a word without a record: never asked)
    for o in sorted(label):
        if label[o][2] not in scenes:
            scenes.append(label[o][2])
        label_of[o] = scenes.index(label[o][2])
    keys, members_of, in_meta = membership(names, meta, by)
    found, cells, words = groups(recs, len(names), n_script, members_of, len(keys), label_of,
                                 len(scenes), min_words, max_gap, min_works)
    gtab = [GROUP_FIELDS]
    for key, n_meta, d in zip(keys, in_meta, found):
        gtab.append([key, n_meta, d['n_works'], d['n_passage_works'], d['n_words'], d['n_exact'],
                     d['n_passages'], d['passage_words'], d['longest'], d['covered'], d['peak'],
                     '' if d['peak_first'] == NONE else d['peak_first'],
                     '' if d['top_label'] == NONE else scenes[d['top_label']],
                     d['top_label_words']])
    stab = [SCENE_FIELDS] + [[keys[c['group']], scenes[c['label']], c['n_words'], c['n_exact'],
                              c['n_works']] for c in cells]
    unknown = (UNKNOWN_WORD, '', '')
    wtab = [WORD_FIELDS]
    for r in words:
        word, char, scene = label.get(r['orig_ix'], unknown)
        wtab.append([keys[r['group']], r['orig_ix'], word, char, scene, r['n_works']])
    return _csv(gtab), _csv(stab), _csv(wtab)
