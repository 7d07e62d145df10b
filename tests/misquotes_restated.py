"""The `misquotes` contract restated in plain Python, with sets and dicts: the oracle of the
tests (tests/test_misquotes_host.py, tests/test_gpu_misquotes.py) and of the committed
tests/golden/misquotes_lines.*.csv.  Passages come from the rule of tests/passages_restated.py.
The product never imports it, and it imports nothing of the product."""

import csv
import io

from tests import passages_restated as pr

NONE = 0xFFFFFFFF
MAX_SCRIPT = 1 << 19
MAX_ROWS = 1 << 27
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
MISQUOTE_KEYS = ['orig_ix', 'spell', 'records', 'works', 'readers', 'telling', 'weight',
                 'first_work']
PAIR_KEYS = ['a', 'b', 'shared', 'score', 'a_on_common', 'b_on_common', 'strongest',
             'strongest_weight']
WORK_KEYS = ['passage_records', 'departures', 'misquotes', 'telling', 'singular', 'partners',
             'closest', 'closest_score']


def is_telling(works, readers, max_share=50):
    """A listed misquote `works` of the `readers` works quoting its script word share."""
    return works * 100 <= max_share * readers


def weight_of(works, readers, weight='rarity'):
    """The weight of a telling misquote."""
    if weight not in ('rarity', 'flat'):
        raise ValueError("weight is rarity or flat")
    return 1 if weight == 'flat' else (readers // works).bit_length()


def agreement(shared, a_on_common, b_on_common):
    return shared * 100 // (a_on_common + b_on_common - shared)


def misquotes(records, same, n_works, n_spell, min_words=6, max_gap=0, min_works=2,
              max_share=50, weight='rarity', min_shared=1, min_score=1):
    """records: (work, fan_ix, orig_ix, spell) sorted by (work, fan_ix); same[o]: the spelling
    that is script word o, NONE for none.  Returns (one dict of WORK_KEYS per work, one dict of
    MISQUOTE_KEYS per listed misquote in the order of their numbers, one dict of PAIR_KEYS per
    kept pair in (a, b) order)."""
    n_script = len(same)
    if min_words < 1 or max_gap < 0 or min_works < 2 or not 1 <= max_share <= 100 \
            or min_shared < 1 or min_score < 1 or weight not in ('rarity', 'flat'):
        raise ValueError("an option out of bounds")
    if len(records) >= MAX_ROWS or n_script > MAX_SCRIPT:
        raise NotImplementedError("too many records, or too long a script")
    for w, _, o, s in records:
        if not (0 <= w < n_works and 0 <= o < n_script and 0 <= s < n_spell):
            raise ValueError("a work, orig_ix or spell out of range")
    if any(s != NONE and not 0 <= s < n_spell for s in same):
        raise ValueError("a same[] out of range")
    found = pr.passages([(w, f, o, 0.0, 0.0) for w, f, o, _ in records], min_words, max_gap)
    inside = [r for p in found for r in records[p['first']:p['first'] + p['n_words']]]

    readers = {}                                   # o: the works with a record at o
    cells = {}                                     # (o, spell): the works of its departures
    works = [dict(passage_records=0, departures=0, misquotes=0, telling=0, singular=0,
                  partners=0, closest=NONE, closest_score=0) for _ in range(n_works)]
    for w, _, o, s in inside:
        works[w]['passage_records'] += 1
        readers.setdefault(o, set()).add(w)
        if s != same[o]:
            works[w]['departures'] += 1
            cells.setdefault((o, s), []).append(w)
    for ws in cells.values():
        if len(set(ws)) == 1:
            works[ws[0]]['singular'] += 1
    listed = sorted((k for k, ws in cells.items() if len(set(ws)) >= min_works),
                    key=lambda k: (k[0], -len(set(cells[k])), -len(cells[k]), k[1]))
    out_m, has = [], [set() for _ in range(n_works)]       # has[w]: its telling misquotes
    for (o, s) in listed:
        ws = cells[(o, s)]
        k, rd = len(set(ws)), len(readers[o])
        tell = is_telling(k, rd, max_share)
        for w in set(ws):
            works[w]['misquotes'] += 1
            if tell:
                works[w]['telling'] += 1
                has[w].add(len(out_m))
        out_m.append(dict(orig_ix=o, spell=s, records=len(ws), works=k, readers=rd,
                          telling=int(tell), weight=weight_of(k, rd, weight) if tell else 0,
                          first_work=min(ws)))
    out_p = []
    active = [w for w in range(n_works) if works[w]['passage_records']]
    for x, a in enumerate(active):
        for b in active[x + 1:]:
            both = has[a] & has[b]
            score = sum(out_m[m]['weight'] for m in both)
            if len(both) < min_shared or score < min_score:
                continue
            strong = min(both, key=lambda m: (-out_m[m]['weight'], m))
            out_p.append(dict(
                a=a, b=b, shared=len(both), score=score,
                a_on_common=sum(1 for m in has[a] if b in readers[out_m[m]['orig_ix']]),
                b_on_common=sum(1 for m in has[b] if a in readers[out_m[m]['orig_ix']]),
                strongest=strong, strongest_weight=out_m[strong]['weight']))
    for p in out_p:
        for me, other in ((p['a'], p['b']), (p['b'], p['a'])):
            v = works[me]
            v['partners'] += 1
            if v['closest'] == NONE or (p['score'], -other) > (v['closest_score'], -v['closest']):
                v['closest'], v['closest_score'] = other, p['score']
    return works, out_m, out_p


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def misquotes_csv(text, min_words=6, max_gap=0, min_works=2, max_share=50, weight='rarity',
                  min_shared=1, min_score=1, keep_case=False):
    """The bytes `ao3.py misquotes` writes for a match CSV's text: (misquotes, misquotes-pairs,
    misquotes-works)."""
    rows = pr.read_rows(text)

    def fold(t):
        return t if keep_case else t.lower()
    label, work_of, spell_of, shown, keyed = {}, {}, {}, [], []
    for k, r in enumerate(rows):
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        have = label.setdefault(o, lab)
        if have != lab:
            what = next(n for n, x, y in zip(('word', 'character', 'scene'), have, lab) if x != y)
            raise ValueError("script word %d has two %ss" % (o, what))
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
        if spell_of.setdefault(fold(r[2]), len(spell_of)) == len(shown):
            shown.append(r[2])                       # as its first appearance wrote it
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4]), spell_of[fold(rows[k][2])]) for w, f, k in keyed]
    n_script = max(label) + 1 if label else 0
    same = [spell_of.get(fold(label[o][0]), NONE) if o in label else NONE
            for o in range(n_script)]
    names = list(work_of)
    works, found, pairs = misquotes(recs, same, len(names), len(spell_of), min_words, max_gap,
                                    min_works, max_share, weight, min_shared, min_score)
    mtab = [MISQUOTE_FIELDS]
    for m in found:
        k = m['works']
        mtab.append([m['orig_ix']] + list(label[m['orig_ix']]) +
                    [shown[m['spell']], m['records'], k, m['readers'], k * 100 // m['readers'],
                     m['telling'], m['weight'], k * (k - 1) // 2 if m['telling'] else 0,
                     names[m['first_work']]])
    ptab = [PAIR_FIELDS]
    for p in sorted(pairs, key=lambda p: (-p['score'], -p['shared'], p['a'], p['b'])):
        s = found[p['strongest']]
        ptab.append([names[p['a']], names[p['b']], p['shared'], p['score'],
                     works[p['a']]['telling'], works[p['b']]['telling'], p['a_on_common'],
                     p['b_on_common'], agreement(p['shared'], p['a_on_common'], p['b_on_common']),
                     s['orig_ix'], label[s['orig_ix']][0], shown[s['spell']], s['works'],
                     s['weight']])
    wtab = [WORK_FIELDS]
    for w, v in enumerate(works):
        if v['passage_records']:
            wtab.append([names[w], v['passage_records'], v['departures'], v['misquotes'],
                         v['telling'], v['singular'], v['partners'],
                         names[v['closest']] if v['partners'] else '', v['closest_score']])
    return _csv(mtab), _csv(ptab), _csv(wtab)
