"""The `works` contract restated in plain Python, work by work: the oracle of the tests
(tests/test_works_host.py, tests/test_gpu_works.py) and of the committed
tests/golden/works_*.csv.  The product never imports it."""

import csv
import io
from collections import Counter

from tests import passages_restated as pr

NONE = 0xFFFFFFFF
THRESHOLDS = [0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
WORK_FIELDS = (['FAN_WORK_FILENAME', 'MATCHED_WORDS', 'EXACT_WORDS',
                'Frequency of Reuse (Exact Matches)'] +
               ['Frequency of Reuse (0-%s)' % t for t in THRESHOLDS[1:]] +
               ['DISTINCT_SCRIPT_WORDS', 'PASSAGES', 'PASSAGE_WORDS', 'LONGEST_PASSAGE',
                'FAN_WORK_WORD_FIRST', 'FAN_WORK_WORD_LAST',
                'SCENES', 'TOP_SCENE', 'TOP_SCENE_WORDS',
                'CHARACTERS', 'TOP_CHARACTER', 'TOP_CHARACTER_WORDS'])
SCENE_FIELDS = ['FAN_WORK_FILENAME', 'ORIGINAL_SCRIPT_SCENE', 'MATCHED_WORDS', 'EXACT_WORDS']
CHARACTER_FIELDS = ['FAN_WORK_FILENAME', 'ORIGINAL_SCRIPT_CHARACTER', 'MATCHED_WORDS',
                    'EXACT_WORDS']
WORK_KEYS = ['first', 'n_words', 'fan_first', 'fan_last', 'n_script_words', 'n_passages',
             'passage_words', 'longest', 'n_groups_hit', 'top_group', 'top_group_words']


def works(records, n_works, n_script, group_of=None, n_groups=0, min_words=6, max_gap=0,
          thresholds=THRESHOLDS):
    """records: (work, fan_ix, orig_ix, dist, comb) tuples sorted by (work, fan_ix).
    Returns (one dict of WORK_KEYS per work, counts[n_works][len(thresholds) + 1],
    cells (work, group, n_words, n_exact) sorted by (work, group))."""
    if min_words < 1:
        raise ValueError("min_words must be at least 1")
    if group_of is not None:
        if len(group_of) != n_script or any(g >= n_groups for g in group_of):
            raise ValueError("group_of outside the groups")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    found = pr.passages(records, min_words, max_gap)         # (raises on unsorted records)
    by_work = [[] for _ in range(n_works)]
    for i, r in enumerate(records):
        by_work[r[0]].append(i)
    spans = [[] for _ in range(n_works)]
    for p in found:
        spans[records[p['first']][0]].append(p['n_words'])
    out, counts, cells = [], [], []
    for w, idx in enumerate(by_work):
        recs = [records[i] for i in idx]
        d = dict.fromkeys(WORK_KEYS, 0)
        d['top_group'] = NONE
        counts.append([sum(1 for r in recs if r[4] <= t) for t in thresholds] + [len(recs)])
        if recs:
            d.update(first=idx[0], n_words=len(recs), fan_first=min(r[1] for r in recs),
                     fan_last=max(r[1] for r in recs),
                     n_script_words=len(set(r[2] for r in recs)),
                     n_passages=len(spans[w]), passage_words=sum(spans[w]),
                     longest=max(spans[w], default=0))
            if group_of is not None:
                per = Counter(group_of[r[2]] for r in recs)
                exact = Counter(group_of[r[2]] for r in recs if r[4] <= 0)
                top = min(per, key=lambda g: (-per[g], g))
                d.update(n_groups_hit=len(per), top_group=top, top_group_words=per[top])
                cells += [(w, g, per[g], exact[g]) for g in sorted(per)]
        out.append(d)
    return out, counts, cells


def label_groups(origs, labels):
    """Labels numbered by the smallest script word index they occur at:
    (group_of[max index + 1], names)."""
    first = {}
    for o, lab in zip(origs, labels):
        first[lab] = min(o, first.get(lab, o))
    names = sorted(first, key=lambda lab: first[lab])
    ident = {lab: k for k, lab in enumerate(names)}
    group_of = [0] * (max(origs) + 1 if origs else 0)
    seen = {}
    for o, lab in zip(origs, labels):
        if seen.setdefault(o, lab) != lab:
            raise ValueError("script word %d has two labels" % o)
        group_of[o] = ident[lab]
    return group_of, names


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def works_csv(text, min_words=6, max_gap=0):
    """The bytes `ao3.py works` writes for a match CSV's text:
    (works, works-scenes, works-characters)."""
    rows = pr.read_rows(text)
    work_of = {}
    keyed = []
    for k, r in enumerate(rows):
        w = work_of.setdefault(r[0], len(work_of))
        keyed.append((w, int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    srt = [rows[k] for _, _, k in keyed]
    recs = [(w, f, int(rows[k][4]), pr._num(rows[k][9]), pr._num(rows[k][11]))
            for w, f, k in keyed]
    origs = [r[2] for r in recs]
    names = list(work_of)
    n_script = max(origs) + 1 if origs else 0
    res = []
    for col in (8, 7):                                # scene, character
        group_of, labels = label_groups(origs, [r[col] for r in srt])
        res.append((labels,) + works(recs, len(names), n_script, group_of, len(labels),
                                     min_words, max_gap))
    (scenes, ws, counts, scells), (chars, wc, _, ccells) = res
    table = [WORK_FIELDS]
    for w, name in enumerate(names):
        a, b = ws[w], wc[w]
        table.append([name, a['n_words'], counts[w][0]] + counts[w][:len(THRESHOLDS)] +
                     [a['n_script_words'], a['n_passages'], a['passage_words'], a['longest'],
                      a['fan_first'], a['fan_last'],
                      a['n_groups_hit'], scenes[a['top_group']], a['top_group_words'],
                      b['n_groups_hit'], chars[b['top_group']], b['top_group_words']])
    out = [_csv(table)]
    for head, labels, cells in ((SCENE_FIELDS, scenes, scells), (CHARACTER_FIELDS, chars, ccells)):
        out.append(_csv([head] + [[names[w], labels[g], n, x] for w, g, n, x in cells]))
    return tuple(out)
