"""The `companions` contract restated in plain Python on tests/passages_restated.py: a set of
script words per work, a set of works per unit, the pair rule on those sets.  The oracle of
tests/test_companions_host.py and tests/test_gpu_companions.py and of the committed
tests/golden/companions_*.csv.  The product never imports it."""

import csv
import io

from tests import passages_restated as pr

NONE = 0xFFFFFFFF
PAIR_FIELDS = ['A', 'B', 'A_FIRST_WORD_INDEX', 'A_LAST_WORD_INDEX', 'A_CHARACTER', 'A_SCENE',
               'A_WORKS', 'B_FIRST_WORD_INDEX', 'B_LAST_WORD_INDEX', 'B_CHARACTER', 'B_SCENE',
               'B_WORKS', 'BOTH', 'EITHER', 'JACCARD_PERCENT', 'SHARE_PERCENT', 'LIFT_PERMILLE',
               'FIRST_FAN_WORK_FILENAME', 'A_TEXT', 'B_TEXT']
UNIT_FIELDS = ['UNIT', 'FIRST_WORD_INDEX', 'LAST_WORD_INDEX', 'CHARACTER', 'SCENE', 'WORKS',
               'PARTNERS', 'BEST_PARTNER', 'BEST_BOTH', 'TEXT']
UNIT_KEYS = ['works', 'partners', 'best', 'best_both']
PAIR_KEYS = ['a', 'b', 'both', 'works_a', 'works_b', 'first_work', 'last_work']
UNKNOWN_WORD = '[?]'


def coverage(records, n_works, min_words=6, max_gap=0):
    """The set of script words the passages of each work cover, bridged words included."""
    cov = [set() for _ in range(n_works)]
    recs = [tuple(r[:3]) + (0.0, 0.0) for r in records]      # (distances play no part)
    for p in pr.passages(recs, min_words, max_gap):          # (raises on unsorted records)
        a, b = recs[p['first']], recs[p['first'] + p['n_words'] - 1]
        cov[a[0]].update(range(a[2], b[2] + 1))
    return cov


def regions_of(cov, n_script, min_works=1):
    """unit_of and the (first, last) of each region: the maximal stretches of script words that
    at least min_works works cover, numbered in script order."""
    depth = [0] * n_script
    for c in cov:
        for o in c:
            depth[o] += 1
    unit_of, bounds = [NONE] * n_script, []
    for o in range(n_script):
        if depth[o] < min_works:
            continue
        if o and unit_of[o - 1] != NONE:
            bounds[-1][1] = o
        else:
            bounds.append([o, o])
        unit_of[o] = len(bounds) - 1
    return unit_of, [tuple(b) for b in bounds]


def labels_of(label_at, n_script):
    """unit_of and the names of the labels {script word: label}, numbered by the first script
    word each occurs at; a script word without a label has no unit."""
    ids, unit_of = {}, [NONE] * n_script
    for o in sorted(label_at):
        unit_of[o] = ids.setdefault(label_at[o], len(ids))
    return unit_of, list(ids)


def companions(records, n_works, n_script, unit_of, n_units, min_words=6, max_gap=0, min_both=2,
               min_share=0):
    """records: (work, fan_ix, orig_ix, ...) tuples sorted by (work, fan_ix).
    Returns (one dict of UNIT_KEYS per unit, one dict of PAIR_KEYS per kept pair in (a, b)
    order)."""
    if min_words < 1 or min_both < 1 or not 0 <= min_share <= 100:
        raise ValueError("min_words and min_both must be at least 1, min_share 0 to 100")
    if len(records) >= 1 << 32:
        raise NotImplementedError("too many records")
    if len(unit_of) != n_script or any(u != NONE and not 0 <= u < n_units for u in unit_of):
        raise ValueError("a unit outside the units")
    for r in records:
        if r[0] >= n_works or r[2] >= n_script:
            raise ValueError("record outside the works or the script")
    cov = coverage(records, n_works, min_words, max_gap)
    members = [set() for _ in range(n_units)]
    for w, c in enumerate(cov):
        for o in c:
            if unit_of[o] != NONE:
                members[unit_of[o]].add(w)
    units = [dict(works=len(m), partners=0, best=NONE, best_both=0) for m in members]
    out = []
    for a in range(n_units):
        for b in range(a + 1, n_units):
            both = members[a] & members[b]
            n, least = len(both), min(len(members[a]), len(members[b]))
            if n < min_both or n * 100 < min_share * least:
                continue
            out.append(dict(a=a, b=b, both=n, works_a=len(members[a]), works_b=len(members[b]),
                            first_work=min(both), last_work=max(both)))
            for u, other in ((a, b), (b, a)):
                units[u]['partners'] += 1
                # the largest both, the smaller unit number on a tie
                if (n, -other) > (units[u]['best_both'], -units[u]['best']):
                    units[u]['best'], units[u]['best_both'] = other, n
    return units, out


def _csv(rows):
    buf = io.StringIO(newline='')
    csv.writer(buf).writerows(rows)
    return buf.getvalue()


def companions_csv(text, by='region', min_words=6, max_gap=0, min_works=1, min_both=2,
                   min_share=0):
    """The bytes `ao3.py companions` writes for a match CSV's text: (companions,
    companions-units)."""
    rows = pr.read_rows(text)
    work_of, keyed = {}, []
    for k, r in enumerate(rows):
        keyed.append((work_of.setdefault(r[0], len(work_of)), int(r[1]), k))
    keyed.sort(key=lambda t: (t[0], t[1]))           # stable: ties keep file order
    recs = [(w, f, int(rows[k][4])) for w, f, k in keyed]
    names = list(work_of)
    label = {}
    for r in rows:
        o, lab = int(r[4]), (r[5], r[7], r[8])       # word, character, scene
        have = label.setdefault(o, lab)
        if have != lab:
            what = next(n for n, x, y in zip(('word', 'character', 'scene'), have, lab) if x != y)
            raise ValueError("script word %d has two %ss" % (o, what))
    n_script = max(label) + 1 if label else 0
    cov = coverage(recs, len(names), min_words, max_gap)
    n_active = sum(1 for c in cov if c)

    def text_of(o):
        return label[o][0] if o in label else UNKNOWN_WORD
    if by == 'region':
        unit_of, bounds = regions_of(cov, n_script, min_works)
        about = [(a, b, label[a][1], label[a][2], ' '.join(text_of(o) for o in range(a, b + 1)))
                 for a, b in bounds]                 # a region starts at a record
    else:
        col = {'character': 1, 'scene': 2}[by]
        unit_of, found = labels_of({o: lab[col] for o, lab in label.items()}, n_script)
        about = []
        for u, name in enumerate(found):
            at = [o for o in range(n_script) if unit_of[o] == u]
            about.append((min(at), max(at), name if col == 1 else '', name if col == 2 else '', ''))
    units, found = companions(recs, len(names), n_script, unit_of, len(about), min_words, max_gap,
                              min_both, min_share)
    ptab = [PAIR_FIELDS]
    for p in sorted(found, key=lambda p: (-p['both'], p['a'], p['b'])):
        a, b, n, wa, wb = p['a'], p['b'], p['both'], p['works_a'], p['works_b']
        either = wa + wb - n
        ptab.append([a + 1, b + 1] + list(about[a][:4]) + [wa] + list(about[b][:4]) + [wb]
                    + [n, either, n * 100 // either, n * 100 // min(wa, wb),
                       n * n_active * 1000 // (wa * wb), names[p['first_work']],
                       about[a][4], about[b][4]])
    utab = [UNIT_FIELDS]
    for u, v in enumerate(units):
        utab.append([u + 1] + list(about[u][:4])
                    + [v['works'], v['partners'], '' if v['best'] == NONE else v['best'] + 1,
                       v['best_both'], about[u][4]])
    return _csv(ptab), _csv(utab)
